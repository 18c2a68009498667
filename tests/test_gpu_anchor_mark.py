"""MI355X: candidate lists from the anchors (csrc/filter.hip 2f) through the context.  A stateless pruning search of the
resident samples that is seeded from the anchor buckets now also takes its lists from them (anchor_mark_kernel and the
per-load run table); tests/test_gpu_anchor_seeds.py's cases run through it unchanged.  Here: the run table the context
builds is NumPy's for the buckets it reads back; the lists are no longer than 1.25 x those of the seed pre-pass
(`anchor_seeds = 0`: prune_mark_kernel over the whole grid, the launches of the parent commit); three frozen and three
evolving epochs are the all-pairs search's bit for bit, with sample weights that hold zeros too."""
import numpy as np
import pytest

from tests import anchor_mark as am
from tests import golden_inputs as gi
from tests import test_gpu_anchor_seeds as tas

pytestmark = pytest.mark.gpu


def _anchored_epochs(X, W0, M, storage=None, n=4):
    be = tas._backend(X, "filtered", 1, storage)
    gamma, hop = tas._gamma(X), gi.lattice_hops(*tas.MAPS[M])
    for _ in range(n):
        be.epoch(W0, hop, tas.SIGMA, gamma, "compact", False)
        assert be.filter_log[-1][0] == "filtered" and be.filter_log[-1][2] == 0
    return be


@pytest.mark.parametrize("storage", ["float32", "bf16"])
@pytest.mark.parametrize("N", [200, 1000, 4096])
def test_run_table_of_the_context(N, storage):
    import bench

    X = bench.make_shard_numpy(N, 70, 4000 + N)
    W0 = tas._map_from(X, 130)
    be = _anchored_epochs(X, W0, 130, storage="bf16" if storage == "bf16" else None)
    assert be.anchor_state == 1 and be.anchor_builds == 1 and be.anchor_searches >= 1
    got, runs = be.read_anchors(), be.read_anchor_runs()
    Xp = np.zeros((N, 80))
    from tests import device_abi as da

    Xp[:, :70] = np.asarray(da.widen(da.stored(X, "bf16" if storage == "bf16" else "f32")), dtype=np.float64)
    ref = am.run_table(Xp, got["anchors"], got["anchor_of"], got["order"])
    assert np.array_equal(runs["run_start"], ref["run_start"]) and np.array_equal(runs["anchor"], ref["anchor"])
    lo, hi = am.widened_R(ref["R2"], 80)
    assert (runs["R"].astype(np.longdouble) >= lo).all() and (runs["R"].astype(np.longdouble) <= hi).all()
    assert np.allclose(runs["xx_max"], ref["xx_max"], rtol=82 * 2.0 ** -52, atol=0) and (runs["xx_max"] > 0).all()
    assert len(runs["anchor"]) <= (N + 127) // 128 + min(N, 256)
    bytes_with = be._get("device_bytes")
    be.anchor_seeds = 0
    be.load(X, storage="bf16" if storage == "bf16" else None)      # other residents: buckets and table are gone
    assert be.anchor_state == 0 and be._get("device_bytes") < bytes_with
    be.release()


def test_lists_no_longer_than_the_pre_pass_leaves():
    """Measured on MI355X: mean list length 39.00 with the seed pre-pass and prune_mark_kernel over the grid, 39.00 with
    the lists from the anchors (one cluster's 32 prototypes, two clusters' where a workgroup straddles a boundary).
    The figures are printed."""
    X, W0 = tas._eight_blobs()
    mean = {}
    for anchors in (0, 1):
        be = tas._backend(X, "filtered", anchors)
        gamma, hop = tas._gamma(X), gi.lattice_hops(*tas.MAPS[256])
        for _ in range(4):
            be.epoch(W0, hop, tas.SIGMA, gamma, "compact", False)
        mean[anchors] = float(be.filter_counts().mean())
        assert be.anchor_state == anchors and (be.anchor_searches >= 1) == bool(anchors)
        be.release()
    print("mean list length: pre-pass %.2f, lists from the anchors %.2f" % (mean[0], mean[1]))
    assert mean[1] <= 1.25 * mean[0]


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "zero_weights"])
def test_frozen_and_evolving_epochs_are_the_all_pairs_search(weighted):
    X, W0 = tas._eight_blobs()
    w = None
    if weighted:
        w = np.random.default_rng(6).uniform(0.0, 2.0, X.shape[0])
        w[::3] = 0.0
    state = tas._three_ways(X, W0, 256, weights=w, frozen=3, evolving=3)
    assert state in (1, 2)   # (_three_ways: the buckets were built and compared epochs took seeds and lists from them)
