"""The topographic function on the MI355X (csrc/topofn.hip): BaseSom.topographic_function / phi against
the reference's results on the golden maps, and the device's histograms and hop distances against the
host default (scipy's unweighted shortest paths) on maps up to M = 4096, irregular lattices and
graphs in several components.  Every comparison is exact."""
import numpy as np
import pytest

from tests.test_topofn_cpu import CASES, check_against_golden, fitted, golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from dbgsom_amd.backend import HipBackend

    be = HipBackend(0)
    yield be
    be.release()


def host(hip, W, X, xy, want_distances=False):
    """The host default (HotPathBackend.topographic_function) with the device's k = 2 search."""
    from dbgsom_amd.backend import HotPathBackend

    return HotPathBackend.topographic_function(hip, W, X, xy, want_distances=want_distances)


def hist_from_D(D, xy):
    """The two histograms implied by a full distance matrix (-1 = unreachable)."""
    xy = np.asarray(xy, dtype=np.int64)
    M = len(xy)
    n_pos = int((xy.max(0) - xy.min(0)).max()) + 1
    i, j = np.nonzero(D == 1)
    hp = np.bincount(np.abs(xy[i] - xy[j]).max(axis=1), minlength=n_pos)
    where = {tuple(p): k for k, p in enumerate(xy.tolist())}
    pairs = [(k, where[(x + dx, y + dy)]) for k, (x, y) in enumerate(xy.tolist())
             for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)) if (x + dx, y + dy) in where]
    a, b = np.array(pairs, dtype=np.int64).T
    t = D[a, b].astype(np.int64)
    hn = np.bincount(np.where(t < 0, M, t), minlength=M + 1)
    return hp, hn


def grid_map(rows, cols, d, n, seed, holes=0.0, shift=(0, 0), clusters=None):
    """A map whose prototypes sit on a jittered rows x cols grid embedded in d dimensions, and n
    samples of the same 2-D sheet (clusters: only around that many random grid points)."""
    rng = np.random.default_rng(seed)
    ii, jj = np.divmod(np.arange(rows * cols), cols)
    keep = rng.random(rows * cols) >= holes
    ii, jj = ii[keep], jj[keep]
    P = rng.normal(size=(2, d))
    W = (np.c_[ii, jj] + rng.uniform(-0.2, 0.2, size=(len(ii), 2))) @ P
    if clusters is None:
        S = rng.uniform(-0.5, [rows - 0.5, cols - 0.5], size=(n, 2))
    else:
        centre = np.c_[ii, jj][rng.choice(len(ii), clusters, replace=False)]
        S = centre[rng.integers(0, clusters, n)] + rng.normal(0, 0.3, size=(n, 2))
    X = (S @ P + rng.normal(0, 0.01, size=(n, d))).astype(np.float32)
    xy = np.c_[ii + shift[0], jj + shift[1]].astype(np.int64)
    return W, X, xy


def check_device_equals_host(hip, W, X, xy):
    hp, hn, D = hip.topographic_function(W, X, xy, want_distances=True)
    rp, rn, RD = host(hip, W, X, xy, want_distances=True)
    assert np.array_equal(D, RD)
    assert np.array_equal(hp, rp) and np.array_equal(hn, rn)
    hp2, hn2, none = hip.topographic_function(W, X, xy)
    assert none is None and np.array_equal(hp2, rp) and np.array_equal(hn2, rn)
    return hp, hn, D


@pytest.mark.parametrize("case", list(CASES))
def test_golden_cases_on_device(hip, case):
    est, X = fitted(case, hip)
    k_pos, k_neg = est.topographic_function(X)
    check_against_golden(est, case, k_pos, k_neg)
    _, _, D = hip.topographic_function(est.weights_, X, est.neurons_, want_distances=True)
    assert np.array_equal(D, golden()[f"{case}_D"])


def test_classifier_and_float32_queries(hip):
    from dbgsom_amd import SomClassifier

    est, X = fitted("digits_clf", hip)
    assert isinstance(est, SomClassifier)
    check_against_golden(est, "digits_clf", *est.topographic_function(X))
    est, X = fitted("digits_f32", hip)
    assert X.dtype == np.float32
    check_against_golden(est, "digits_f32", *est.topographic_function(X))


def test_fit_then_topographic_function_end_to_end():
    from sklearn.datasets import load_digits

    from dbgsom_amd import SomVQ

    X = load_digits().data
    est = SomVQ(random_state=0).fit(X)
    check_against_golden(est, "digits_f64", *est.topographic_function(X))


@pytest.mark.parametrize("rows,cols,n", [(32, 32, 200_000), (64, 64, 200_000)])
def test_device_equals_host_on_grid_maps(hip, rows, cols, n):
    W, X, xy = grid_map(rows, cols, 16, n, seed=rows)
    hp, hn, _ = check_device_equals_host(hip, W, X, xy)
    assert hp.sum() > rows * cols and hn[1] > 0


def test_irregular_lattice_with_holes_and_negative_coordinates(hip):
    W, X, xy = grid_map(40, 40, 12, 60_000, seed=7, holes=0.2, shift=(-17, -23))
    assert xy.min() < 0
    check_device_equals_host(hip, W, X, xy)


def test_several_components(hip):
    W, X, xy = grid_map(30, 30, 12, 20_000, seed=9, clusters=6)
    hp, hn, D = check_device_equals_host(hip, W, X, xy)
    assert hn[-1] > 0 and (D < 0).any()


def test_histogram_mode_equals_full_mode_at_8000(hip):
    W, X, xy = grid_map(80, 100, 16, 200_000, seed=11, holes=0.02)
    assert 7500 < len(xy) <= 8000
    hp, hn, none = hip.topographic_function(W, X, xy)
    fp, fn, D = hip.topographic_function(W, X, xy, want_distances=True)
    assert none is None and np.array_equal(hp, fp) and np.array_equal(hn, fn)
    rp, rn = hist_from_D(D, xy)
    assert np.array_equal(hp, rp) and np.array_equal(hn, rn)


def test_two_calls_bit_identical(hip):
    W, X, xy = grid_map(32, 32, 16, 50_000, seed=3, holes=0.1)
    a = hip.topographic_function(W, X, xy, want_distances=True)
    b = hip.topographic_function(W, X, xy, want_distances=True)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def test_device_path_uses_no_host_graph_code(hip, monkeypatch):
    import networkx
    import scipy.sparse.csgraph

    def boom(*a, **k):
        raise AssertionError("host graph code called")

    monkeypatch.setattr(scipy.sparse.csgraph, "shortest_path", boom)
    monkeypatch.setattr(networkx, "floyd_warshall_numpy", boom)
    est, X = fitted("grow_blobs_f32", hip)
    check_against_golden(est, "grow_blobs_f32", *est.topographic_function(X))
