"""CPU: init="pca" / initial_shape -- the driver of dbgsom_amd/linear_init.py on the NumPy stand-in of the covariance pass,
the grid lattice, the start formula, the estimator surface and its refusals, and the argument errors of the new C calls.
(The kernel itself: tests/test_gpu_linear_init.py.)"""
import inspect
import os
import pickle

import numpy as np
import pytest
import scipy.sparse
from sklearn.base import clone

from dbgsom_amd import SomClassifier, SomVQ, linear_init
from dbgsom_amd.lattice import GrowingLattice
from oracle.som_oracle import OracleBackend
from tests import golden_inputs as gi
from tests import linear_init as li

PLANTED = [(3000, 37, np.float32), (3000, 37, np.float64), (500, 785, np.float32), (257, 2, np.float64),
           (500, 5, np.float32)]


def _plane(X):
    be = li.StandIn().load(X)
    return linear_init.principal_plane(be, X.shape[0], X.shape[1])


@pytest.fixture(scope="module")
def planes():
    out = {}
    for N, d, dt in PLANTED:
        X = li.planted(N, d, seed=N + d, dtype=dt)
        out[(N, d, dt)] = (X, _plane(X), li.reference_spectrum(X))
    return out


# ---- the pass ---------------------------------------------------------------------------------------------------------
def test_shape_table_holds_the_rows_it_claims():
    Ns = {s[0] for s in li.SHAPES}
    assert 1 in Ns and li.CV_MIN_SHARE - 1 in Ns and li.CV_MIN_SHARE + 1 in Ns and max(Ns) <= 20000
    assert all(li.share(N) == li.CV_MIN_SHARE for N in Ns)                      # (what "one fewer / one more" refers to)
    assert any(li.partials(N) > 4 and N % li.share(N) and N % li.CV_R for N in Ns)   # several partials, uneven last step
    assert {1, 2, 63, 64, 65, 785, 4099, li.CV_CHUNK, li.CV_CHUNK + 1} <= {s[1] for s in li.SHAPES}
    assert {s[2] for s in li.SHAPES} == {1, 2, 8} and {s[3] for s in li.SHAPES} == {"zeros", "true"}
    assert li.share(10 ** 6) == 1956 and li.partials(10 ** 6) == 512 and li.share(1) == 64 and li.partials(1) == 1


@pytest.mark.parametrize("N,d,p,mean_kind", li.SHAPES)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_stand_in_within_the_bound_of_the_exact_pass(N, d, p, mean_kind, dtype):
    X, mean, V, Z, s, zb, sb = li.raw_case(N, d, p, mean_kind, dtype)
    got_Z, got_s = li.StandIn().load(X).covariance_apply(mean, V)
    okz, wz = li.within(got_Z, Z, zb)
    oks, ws = li.within(got_s, s, sb)
    print(f"worst |err| / bound: Z {wz:.3g}, colsum {ws:.3g}")
    assert okz and oks
    # the reference alone: rounded to float64 it is within one rounding of itself, far inside the bound
    assert li.within(np.asarray(Z, dtype=np.float64), Z, zb)[0]


# ---- the driver -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", PLANTED, ids=lambda k: f"{k[0]}x{k[1]}-{np.dtype(k[2]).name}")
def test_driver_converges_to_eigh_on_planted_data(planes, key):
    X, plane, (lam, E) = planes[key]
    N, d, _ = key
    print(f"passes {plane.n_passes}, residual {plane.residual:.3g}")
    assert plane.n_passes < linear_init.MAX_PASSES and plane.residual <= linear_init.RESIDUAL_TOL
    if d < linear_init.BLOCK:
        assert plane.n_passes == 1                                            # p = d: the block is the whole space
    np.testing.assert_allclose(plane.mean, np.asarray(X, dtype=np.float64).mean(axis=0), rtol=1e-13)
    np.testing.assert_allclose(plane.variances, lam[:2], rtol=1e-12)
    assert plane.variances[0] >= plane.variances[1] > 0
    for j in range(2):
        err, tol = np.linalg.norm(plane.directions[j] - E[j]), li.direction_tolerance(lam, j)
        print(f"direction {j}: |u - e| = {err:.3g}, tolerance {tol:.3g}")
        assert err <= tol
        assert abs(np.linalg.norm(plane.directions[j]) - 1.0) < 1e-14
        assert plane.directions[j][np.argmax(np.abs(plane.directions[j]))] > 0     # the sign rule


def test_isotropic_data_stops_at_the_cap_without_raising():
    X = li.planted(3000, 37, seed=1, isotropic=True)
    plane = _plane(X)
    assert plane.n_passes == linear_init.MAX_PASSES and plane.residual > linear_init.RESIDUAL_TOL
    assert plane.variances[0] >= plane.variances[1] > 0 and np.isfinite(plane.directions).all()


def test_sign_rule():
    assert np.array_equal(linear_init.fix_sign(np.array([0.5, -2.0, 1.0])), [-0.5, 2.0, -1.0])
    assert np.array_equal(linear_init.fix_sign(np.array([0.5, 2.0, -1.0])), [0.5, 2.0, -1.0])
    assert np.array_equal(linear_init.fix_sign(np.array([-2.0, 2.0, 1.0])), [2.0, -2.0, -1.0])   # tie: the lowest index


# ---- the grid ---------------------------------------------------------------------------------------------------------
def test_grid_lattice():
    rows, cols = 3, 5
    W = np.arange(rows * cols * 2, dtype=np.float64).reshape(rows * cols, 2)
    lat = GrowingLattice.grid(rows, cols, W)
    assert lat.nodes == [(a, b) for a in range(rows) for b in range(cols)]          # row-major
    assert np.array_equal(lat.hop_distances(), gi.lattice_hops(rows, cols))
    ii, jj = np.divmod(np.arange(rows * cols), cols)
    assert np.array_equal(lat.hop_distances(), np.abs(ii[:, None] - ii[None]) + np.abs(jj[:, None] - jj[None]))
    assert lat.graph.number_of_edges() == rows * (cols - 1) + cols * (rows - 1)
    assert all(lat.index_of(n) == i for i, n in enumerate(lat.nodes)) and np.array_equal(lat.W, W)
    assert lat.error.shape == (15,) and not lat.has_error.any() and not lat.epoch_created.any()
    # (2, 2): the start square of __init__, node order and adjacency lists (growth reads their order)
    a, b = GrowingLattice.grid(2, 2, W[:4]), GrowingLattice(W[:4])
    assert a.nodes == b.nodes == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert {n: list(a.graph.adj[n]) for n in a.nodes} == {n: list(b.graph.adj[n]) for n in b.nodes}
    assert a._index == b._index
    for bad in ((1, 4), (4, 1)):
        with pytest.raises(ValueError):
            GrowingLattice.grid(*bad, W[:4])
    with pytest.raises(ValueError):
        GrowingLattice.grid(2, 3, W[:5])


def test_grid_grows_at_the_boundary_as_the_square_does():
    lat = GrowingLattice.grid(3, 3, np.arange(18, dtype=np.float64).reshape(9, 2))
    err = np.zeros(9)
    err[lat.index_of((0, 1))] = 5.0          # a boundary node with one free side
    err[lat.index_of((1, 1))] = 9.0          # the interior node: hands half of its error to the rim
    lat.set_errors(err)
    lat.distribute_errors(1.0)
    assert lat.error[lat.index_of((1, 1))] == 4.5 and lat.error[lat.index_of((0, 1))] == 5.0 + 4.5 / 4
    assert lat.will_grow(1.0)
    assert lat.grow(1.0, epoch=3) >= 1
    assert (-1, 1) in lat.nodes and lat.graph.has_edge((-1, 1), (0, 1))
    assert np.array_equal(lat.weight((-1, 1)), 2 * lat.weight((0, 1)) - lat.weight((1, 1)))
    assert lat.epoch_created[lat.index_of((-1, 1))] == 3


# ---- the estimator ----------------------------------------------------------------------------------------------------
def _X(dtype=np.float32):
    return li.planted(400, 9, seed=11, dtype=dtype)


def _vq(**kw):
    kw.setdefault("n_iter", 12)
    return SomVQ(backend=li.StandIn(), init="pca", **kw)


def test_start_formula_against_numpy(planes):
    X, _, (lam, E) = planes[(3000, 37, np.float32)]
    rows, cols = 4, 3
    est = _vq(initial_shape=(rows, cols), max_neurons=12, n_iter=1)
    seen = {}
    orig = est._start_prototypes

    def spy(data):
        seen["nodes"], seen["W"] = orig(data)
        return seen["nodes"], seen["W"]

    est._start_prototypes = spy
    est.fit(X)
    mu, (e1, e2), (l1, l2) = est.init_mean_, est.init_directions_, est.init_variances_
    want = np.array([mu + (2 * a / (rows - 1) - 1) * np.sqrt(l1) * e1 + (2 * b / (cols - 1) - 1) * np.sqrt(l2) * e2
                     for a in range(rows) for b in range(cols)])
    assert seen["nodes"] == [(a, b) for a in range(rows) for b in range(cols)]
    assert seen["W"].dtype == np.float64                       # float64 for float32 X too
    np.testing.assert_allclose(seen["W"], want, rtol=1e-14, atol=1e-13)
    assert est.init_mean_.shape == (37,) and est.init_directions_.shape == (2, 37) and est.init_variances_.shape == (2,)
    assert est.init_n_passes_ >= 1
    for j in range(2):
        assert np.linalg.norm(est.init_directions_[j] - E[j]) <= li.direction_tolerance(lam, j)
    # the corners of the grid are mean +- sqrt(l1) e1 +- sqrt(l2) e2
    np.testing.assert_allclose(seen["W"][0], mu - np.sqrt(l1) * e1 - np.sqrt(l2) * e2, rtol=1e-14, atol=1e-13)


def test_fixed_grid_keeps_its_shape_and_a_larger_budget_grows():
    X = _X()
    fixed = _vq(initial_shape=(3, 4), max_neurons=12).fit(X)
    assert len(fixed.neurons_) <= 12 and set(fixed.neurons_) <= {(a, b) for a in range(3) for b in range(4)}
    assert not any(d["epoch_created"] for _, d in fixed.som_.nodes.data())
    assert fixed.weights_.shape[1] == 9 and fixed.labels_.shape == (400,)
    grown = _vq(initial_shape=(2, 3), max_neurons=40, spreading_factor=0.9, n_iter=20).fit(X)
    assert not set(grown.neurons_) <= {(a, b) for a in range(2) for b in range(3)}
    assert any(d["epoch_created"] for _, d in grown.som_.nodes.data())


def test_start_does_not_depend_on_random_state_and_fits_repeat():
    X = _X()
    a = _vq(initial_shape=(3, 3), max_neurons=9, random_state=0).fit(X)
    b = _vq(initial_shape=(3, 3), max_neurons=9, random_state=77).fit(X)
    c = _vq(initial_shape=(3, 3), max_neurons=9, random_state=None).fit(X)
    assert np.array_equal(a.weights_, b.weights_) and np.array_equal(a.weights_, c.weights_)
    assert a.neurons_ == b.neurons_ and np.array_equal(a.labels_, b.labels_)
    assert np.array_equal(a.init_directions_, b.init_directions_) and a.init_n_passes_ == b.init_n_passes_
    lin = SomVQ(backend=li.StandIn(), init="linear", initial_shape=(3, 3), max_neurons=9, n_iter=12).fit(X)
    assert np.array_equal(lin.weights_, a.weights_)            # the alias


def test_float32_and_float64_rows_give_the_same_start_up_to_the_rows_rounding():
    X64 = _X(np.float64)
    a, b = _vq(n_iter=1).fit(X64), _vq(n_iter=1).fit(X64.astype(np.float32))
    np.testing.assert_allclose(a.init_variances_, b.init_variances_, rtol=1e-5)
    np.testing.assert_allclose(a.init_directions_, b.init_directions_, atol=1e-5)


def test_classifier_takes_the_parameters_too():
    X = _X()
    y = (X[:, 0] > np.median(X[:, 0])).astype(int)
    clf = SomClassifier(backend=li.StandIn(), init="pca", initial_shape=(3, 3), max_neurons=9, n_iter=10).fit(X, y)
    assert hasattr(clf, "init_directions_") and clf.predict(X).shape == (400,)


def test_sklearn_round_trips_and_signature():
    names = list(inspect.signature(SomVQ.__init__).parameters)
    assert names[-1] == "missing_values" and names[-3:-1] == ["init", "initial_shape"]
    assert names[names.index("init") - 1] == "sharded_input"
    est = SomVQ()
    assert est.init == "random" and est.initial_shape == (2, 2)
    assert est.get_params()["init"] == "random" and est.get_params()["initial_shape"] == (2, 2)
    fitted = _vq(initial_shape=(3, 4), max_neurons=12).fit(_X())
    c = clone(fitted)
    assert c.init == "pca" and c.initial_shape == (3, 4) and not hasattr(c, "init_mean_")
    back = pickle.loads(pickle.dumps(fitted))
    assert back.init == "pca" and back.initial_shape == (3, 4)
    assert np.array_equal(back.init_directions_, fitted.init_directions_) and back.init_n_passes_ == fitted.init_n_passes_
    assert np.array_equal(back.weights_, fitted.weights_)
    # the attributes exist only under init="pca": a refit with init="random" drops them
    fitted.set_params(init="random", initial_shape=(2, 2)).fit(_X())
    assert not any(hasattr(fitted, n) for n in ("init_mean_", "init_directions_", "init_variances_", "init_n_passes_"))


def test_random_init_is_the_parent_commits_fit_bit_for_bit(golden_dir):
    """tests/golden/linear_init_parent.npz: ``SomVQ(backend=OracleBackend(), random_state=3, n_iter=30,
    max_neurons=30).fit(X)`` on ``golden_inputs.blobs_f32(600, 12, seed=5)`` as float32 and as float64, recorded at the
    commit before ``init`` existed."""
    g = np.load(os.path.join(golden_dir, "linear_init_parent.npz"))
    for tag, dt in (("f32", np.float32), ("f64", np.float64)):
        X = np.ascontiguousarray(gi.blobs_f32(600, 12, seed=5)[0], dtype=dt)
        est = SomVQ(backend=OracleBackend(), random_state=3, n_iter=30, max_neurons=30).fit(X)
        assert est.n_iter_ == int(g[tag + "_n_iter"])
        assert est.neurons_ == [tuple(n) for n in g[tag + "_neurons"]]
        assert np.array_equal(est.weights_, g[tag + "_weights"])
        assert not hasattr(est, "init_mean_")


def test_an_injected_start_is_what_the_fit_starts_from():
    X = _X()
    W0 = np.asarray(X[:6], dtype=np.float64)
    est = SomVQ(backend=OracleBackend(), n_iter=1, max_neurons=6)
    est._start_prototypes = lambda data: ([(a, b) for a in range(2) for b in range(3)], W0)
    seen = []
    orig = est._grow_som
    est._grow_som = lambda data, y: (seen.append((list(est.neurons_), est.weights_.copy())), orig(data, y))[1]
    est.fit(X)
    assert seen[0][0] == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)] and np.array_equal(seen[0][1], W0)


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals():
    X = _X()
    bogus = SomVQ(backend=li.StandIn(), init="bogus", n_iter=3)                 # (no error in __init__)
    with pytest.raises(ValueError, match="init must be"):
        bogus.fit(X)
    with pytest.raises(ValueError, match=r"initial_shape.*init"):
        SomVQ(backend=li.StandIn(), initial_shape=(3, 3), n_iter=3).fit(X)
    for shape in ((1, 3), (3,), (2.5, 3), "ab", 4, (2, 2, 2), (True, 3)):
        with pytest.raises(ValueError, match="initial_shape"):
            _vq(initial_shape=shape).fit(X)
    pca = 'init="pca"'
    loaded = []

    class NoLoad(li.StandIn):
        def load(self, X):
            loaded.append(1)
            return super().load(X)

    def vq(**kw):
        return SomVQ(backend=NoLoad(), init="pca", n_iter=3, **kw)

    with pytest.raises(ValueError, match=pca + ".*sparse"):
        vq().fit(scipy.sparse.csr_matrix(X))
    Xn = X.copy()
    Xn[3, 2] = np.nan
    with pytest.raises(ValueError, match=pca + ".*missing"):
        vq(missing_values="nan-fit").fit(Xn)
    with pytest.raises(ValueError, match=pca + ".*sample_weight"):
        vq().fit(X, sample_weight=np.ones(len(X)))
    with pytest.raises(ValueError, match=pca + ".*vertical_growth"):
        vq(vertical_growth=True).fit(X)
    with pytest.raises(ValueError, match=pca + ".*sharded_input"):
        vq(sharded_input=True).fit(X)
    assert not loaded                                                           # before anything is uploaded
    with pytest.raises(ValueError, match=pca + ".*fewer than two directions of variance"):
        vq().fit(np.ones((20, 5)))
    with pytest.raises(ValueError, match=pca + ".*fewer than two directions of variance"):
        vq().fit(np.arange(20.0)[:, None])
    # complete rows under "nan-fit" are an ordinary fit: allowed
    assert hasattr(vq(missing_values="nan-fit").fit(X), "init_mean_")
    # a backend without the call: no quiet fallback
    with pytest.raises(NotImplementedError, match="covariance_apply"):
        SomVQ(backend=OracleBackend(), init="pca", n_iter=3).fit(X)
    # metric is free: the start does not depend on the search (the stand-in has no L1 epoch, so only up to the start)
    est = SomVQ(backend=li.StandIn(), init="pca", metric="chebyshev", n_iter=2).fit(X)
    assert hasattr(est, "init_mean_")


# ---- the C calls ------------------------------------------------------------------------------------------------------
def test_argument_errors_of_the_new_calls_are_status_codes():
    from dbgsom_amd import _native

    lib = _native.load()
    ws = lib.dbgsom_covariance_apply_workspace_bytes
    assert _native.MAX_DIRECTIONS == li.MAX_DIRECTIONS == linear_init.BLOCK == 8
    assert ws(0, 4, 1) == 0 and ws(10, 0, 1) == 0 and ws(10, 4, 0) == 0 and ws(10, 4, 9) == 0
    for N, d in ((1, 1), (63, 7), (65, 7), (1000, 785), (10 ** 6, 784)):
        assert ws(N, d, 8) == ws(N, d, 1) == li.partials(N) * 9 * d * 8
    one = 8   # (never dereferenced: every call below fails before a launch)

    def call(x_dtype=0, N=10, d=4, ldx=4, V=one, p=2, Z=one, s=one, w=one, wb=1 << 20, X=one):
        return lib.dbgsom_covariance_apply(X, x_dtype, N, d, ldx, None, V, p, Z, s, w, wb, None)

    for kw, word in ((dict(x_dtype=2), b"float32 / float64"), (dict(x_dtype=7), b"x_dtype"), (dict(p=0), b"p must be"),
                     (dict(p=9), b"p must be"), (dict(d=0), b"bad shape"), (dict(ldx=3), b"bad shape"),
                     (dict(N=-1), b"bad shape"), (dict(V=None), b"null"), (dict(Z=None), b"null"), (dict(s=None), b"null"),
                     (dict(X=None), b"null")):
        assert call(**kw) == -1 and word in lib.dbgsom_last_error(), kw
    assert call(wb=ws(10, 4, 2) - 1) == -3 and b"workspace too small" in lib.dbgsom_last_error()
    assert call(w=None) == -3
    assert lib.dbgsom_ctx_covariance_apply(None, None, None, 2, None, None) == -1
    assert b"null context" in lib.dbgsom_last_error()
