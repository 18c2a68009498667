"""MI355X: the lean form of the anchor-seeded epoch through the context (csrc/lean_gate.h, DBGSOM_ANCHOR_LISTS_ONLY).
Behind an anchor-seeded epoch that handed nothing to the per-sample pass, the next epoch on the same samples, map size
and plan makes nothing for that pass: no digit planes of W, no gap table, no per-sample seeds.  The guess can only cost
time: winners, distances, new prototypes, errors and activations of every epoch here are the all-pairs search's bit for
bit, and `lean_searches` says which epochs took the form.

Blobs 8 cluster radii apart (tests/anchor_mark.py): a list is one cluster's prototypes, nothing is handed over.
Clusters 2.5 radii apart: every workgroup is handed over (tests/test_gpu_anchor_mark_device.py records it) and no epoch
may be lean.  `sweep_planes = 4`, `seed_stride = 4` as in tests/test_gpu_anchor_seeds.py: the pruning form on the cheap
seeds the anchors replace."""
import numpy as np
import pytest

from tests import anchor_mark as am
from tests import golden_inputs as gi
from tests import test_gpu_anchor_seeds as tas

pytestmark = pytest.mark.gpu

SIGMA = tas.SIGMA
# evolving maps: these maps are drawn from the samples in no lattice order, and a neighbourhood of 1.1 hops averages
# prototypes of different clusters into the middle, where every list is the whole map and nothing is ever lean; a narrow
# one (a neighbour's weight exp(-1 / 0.18) = 0.004) moves every prototype to the mean of its own samples
SIGMA_EVOLVING = 0.3
# (N, d, M, storage): d = 48 is padded to 64 and d = 70 to 80 on the device; one shape per storage type
SHAPES = [(4096, 48, 130, "float32"), (1000, 70, 256, "float64"), (4096, 70, 256, "bf16")]


def _hop(M):
    return gi.lattice_hops(*tas.MAPS[M]) if M in tas.MAPS else gi.lattice_hops(1, M)


def _inputs(N, d, M, storage, key="lean", radii=8.0):
    X, W0 = am.blobs(N, d, M, key, radii=radii)
    if storage == "float64":
        X = X.astype(np.float64) * (1.0 + 2.0 ** -30)          # (float64 rows that are no float32 values)
    return X, W0


def _backend(X, algorithm, storage):
    return tas._backend(X, algorithm, 1, "bf16" if storage == "bf16" else None)


class _Run:
    """epochs of one backend, every output kept; frozen: the resident map stays (the bench's path), else it evolves"""

    def __init__(self, be, X, W0, frozen):
        self.be, self.gamma, self.frozen, self.W, self.out = be, tas._gamma(X), frozen, W0, []
        self.sigma = SIGMA if frozen else SIGMA_EVOLVING
        if frozen:
            be.set_weights(W0)

    def set_map(self, W):
        self.W = W
        if self.frozen:
            self.be.set_weights(W)

    def epoch(self):
        from dbgsom_amd.backend import RESIDENT

        hop = _hop(self.W.shape[0])
        if self.frozen:
            r = self.be.epoch(RESIDENT, hop, self.sigma, self.gamma, "compact", True, keep_on_device=True, frozen=True)
            Wn = self.be.get_weights(1)
        else:
            r = self.be.epoch(self.W, hop, self.sigma, self.gamma, "compact", True)
            Wn = self.W = r.new_weights
        self.out.append((r.winners, r.distances, Wn, r.errors, r.activations, np.array([r.change_total])))
        if self.be.filter_log and self.be.filter_log[-1][0] == "filtered":
            print(f"  epoch {len(self.out)}: anchor searches {self.be.anchor_searches}, lean {self.be.lean_searches}, "
                  f"re-seeding {self.be._get('prune_retry')}, longest list {int(self.be.filter_counts().max())}")

    def until_anchored(self, limit=4):
        """epochs until one was seeded from the anchors (the pre-pass seeds one or two reference epochs first)
        -> how many ran"""
        before = self.be.anchor_searches
        for n in range(1, limit + 1):
            self.epoch()
            assert self.be.filter_log[-1][0] == "filtered" and self.be.filter_log[-1][2] == 0
            if self.be.anchor_searches > before:
                return n
        raise AssertionError("no epoch was seeded from the anchors")


def _reference(X, W_of_epoch, storage, frozen, n):
    """the same n epochs through the all-pairs search; W_of_epoch: {epoch: map set in front of it}"""
    ref = _Run(_backend(X, "exact", storage), X, W_of_epoch[0], frozen)
    for e in range(n):
        if e and e in W_of_epoch:
            ref.set_map(W_of_epoch[e])
        ref.epoch()
    ref.be.release()
    return ref.out


@pytest.mark.parametrize("frozen", [True, False], ids=["frozen", "evolving"])
@pytest.mark.parametrize("N,d,M,storage", SHAPES, ids=[f"N{s[0]}-d{s[1]}-M{s[2]}-{s[3]}" for s in SHAPES])
def test_lean_epochs_are_the_all_pairs_search(N, d, M, storage, frozen):
    X, W0 = _inputs(N, d, M, storage)
    run = _Run(_backend(X, "filtered", storage), X, W0, frozen)
    be = run.be
    n0 = run.until_anchored()
    assert be.lean_searches == 0, "the first anchor-seeded epoch is a full one"
    assert be.anchor_state == 1
    counts_full, searches = be.filter_counts().copy(), be.anchor_searches
    for k in range(1, 5):
        run.epoch()
        assert be.anchor_state == 1 and be.anchor_searches == searches + k
        assert be.lean_searches == k, (k, be.lean_searches)
        if frozen:                       # the same map: the lean epoch's lists are the full epoch's
            assert np.array_equal(be.filter_counts(), counts_full)
    print(f"N={N} d={d} M={M} {storage} {'frozen' if frozen else 'evolving'}: anchors from epoch {n0}, "
          f"mean list {counts_full.mean():.1f}, {be.lean_searches} lean epochs")
    assert counts_full.max() <= am.long_above(M)
    be.release()
    assert tas._same(run.out, _reference(X, {0: W0}, storage, frozen, n0 + 4)), "not the all-pairs search's results"


def test_never_lean_while_lists_are_handed_over():
    N, d, M, storage = 4096, 70, 256, "float32"
    X, W0 = am.blobs(N, d, M, "close", radii=2.5)
    run = _Run(_backend(X, "filtered", storage), X, W0, True)
    for _ in range(6):
        run.epoch()
        assert run.be.filter_log[-1][0] == "filtered"
        assert run.be.lean_searches == 0
    print(f"anchor searches {run.be.anchor_searches}, anchor state {run.be.anchor_state}, "
          f"mean list {run.be.filter_counts().mean():.1f} of {M}")
    run.be.release()
    assert tas._same(run.out, _reference(X, {0: W0}, storage, True, 6))


def test_a_wrong_guess_costs_only_time():
    N, d, M, storage = 4096, 48, 130, "float32"
    X, W0 = _inputs(N, d, M, storage)
    run = _Run(_backend(X, "filtered", storage), X, W0, True)
    be = run.be
    n0 = run.until_anchored()
    run.epoch()
    assert be.lean_searches == 1
    # a map of the same size whose rows are noisy copies of ONE cluster's prototype: from every anchor all of them
    # are about as far, and every list is the whole map
    rng = am.rng_for("one_cluster")
    W1 = np.ascontiguousarray(W0[:1] + 0.05 * rng.standard_normal((M, d)))
    run.set_map(W1)
    run.epoch()
    assert be.lean_searches == 2, "the same samples, map size and plan: the guess is made"
    assert be.anchor_state == 1, "a lean epoch that kept long lists is not held against the anchors' valve"
    assert be._get("prune_retry") == 0, "a lean epoch turned the policy's re-seeding on"
    counts = be.filter_counts()
    assert counts.max() > am.long_above(M), "the case kept no long list"
    run.epoch()
    assert be.lean_searches == 2, "the epoch behind a wrong guess is a full one"
    be.release()
    assert tas._same(run.out, _reference(X, {0: W0, n0 + 1: W1}, storage, True, n0 + 3))


def test_growth_and_reload_start_from_a_full_epoch():
    N, d, M, storage = 4096, 48, 130, "float32"
    X, W0 = _inputs(N, d, M, storage)
    run = _Run(_backend(X, "filtered", storage), X, W0, False)
    be = run.be
    n0 = run.until_anchored()
    run.epoch()
    assert be.lean_searches == 1
    # a growth step: one more row
    W1 = np.ascontiguousarray(np.vstack([run.W, run.W[-1:] + 0.01]))
    run.W = W1
    searches = be.anchor_searches
    run.epoch()
    assert be.lean_searches == 1, "the first epoch on M + 1 prototypes is a full one"
    if be.anchor_searches == searches + 1:           # (seeded from the anchors at once: the next one is lean again)
        run.epoch()
        assert be.lean_searches == 2
    n1 = len(run.out)
    ref = _reference(X, {0: W0, n0 + 1: W1}, storage, False, n1)
    assert tas._same(run.out, ref)
    # other residents (the same rows, loaded again): buckets, table and every count are gone
    be.load(X)
    assert be.anchor_state == 0
    lean = be.lean_searches
    run2 = _Run(be, X, W0, False)
    run2.until_anchored()
    assert be.lean_searches == lean, "the first anchor-seeded epoch behind a load is a full one"
    run2.epoch()
    assert be.lean_searches == lean + 1
    be.release()
