"""GPU: device tensors as X.  Every public method that takes complete dense rows takes a torch tensor on the
estimator's GPU and gives the result of the same call on ``X.cpu().numpy()`` bit for bit, without X crossing PCIe.
The oracle everywhere is that host-array call in the same process: both run the same kernels on the same bytes, so
every comparison is ``array_equal`` / ``torch.equal``."""
import numpy as np
import pytest

from tests import golden_inputs as gi

pytestmark = pytest.mark.gpu

FIT_ATTRS = ("weights_", "labels_", "neurons_", "n_iter_", "quantization_error_", "topographic_error_",
             "growing_threshold_")
LAYOUTS = ("borrowed", "d61", "colslice", "offset")
VQ_KW = dict(random_state=0, n_iter=30)


def _torch():
    import torch

    return torch


def _digits(dtype):
    return np.ascontiguousarray(gi.case_X("digits_f64")[0], dtype=dtype)


def _layout(Xh, layout):
    """-> (host array, tensor on cuda:0 holding the same values in the named layout)"""
    torch = _torch()
    n, d = Xh.shape
    if layout == "borrowed":      # d % 16 == 0, contiguous rows, 16-byte aligned base: read in place
        t = torch.from_numpy(Xh).cuda()
        assert t.data_ptr() % 16 == 0 and t.stride() == (d, 1) and d % 16 == 0
    elif layout == "d61":         # d no multiple of 16: pad-copied on the device
        Xh = np.ascontiguousarray(Xh[:, :61])
        t = torch.from_numpy(Xh).cuda()
    elif layout == "colslice":    # row stride != padded d
        big = torch.full((n, 80), 7.0, dtype=torch.from_numpy(Xh).dtype, device="cuda")
        big[:, :d] = torch.from_numpy(Xh).cuda()
        t = big[:, :d]
        assert t.stride() == (80, 1)
    elif layout == "offset":      # base one element off a 16-byte boundary (4 bytes for float32)
        buf = torch.zeros(n * d + 1, dtype=torch.from_numpy(Xh).dtype, device="cuda")
        t = buf[1:].view(n, d)
        t.copy_(torch.from_numpy(Xh).cuda())
        assert t.data_ptr() % 16 == Xh.itemsize
    else:
        raise KeyError(layout)
    assert np.array_equal(t.cpu().numpy(), Xh)
    return Xh, t


def _same_fit(a, b, attrs=FIT_ATTRS):
    for name in attrs:
        va, vb = getattr(a, name), getattr(b, name)
        assert isinstance(va, type(vb)), name
        if isinstance(vb, np.ndarray):
            assert va.dtype == vb.dtype and np.array_equal(va, vb), name
        else:
            assert va == vb, name


def _node_values(est, attribute):
    return np.array([data[attribute] for _, data in est.som_.nodes.data()])


# -- 1. fit parity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fit_on_a_tensor_is_the_fit_on_its_host_copy(dtype, layout):
    from dbgsom_amd import SomVQ

    Xh, Xt = _layout(_digits(dtype), layout)
    host = SomVQ(**VQ_KW).fit(Xh)
    dev = SomVQ(**VQ_KW).fit(Xt)
    _same_fit(dev, host)
    assert dev.n_features_in_ == Xh.shape[1] and isinstance(dev.labels_, np.ndarray)


# -- 2. classifier fit parity -------------------------------------------------------------------------------------
@pytest.mark.parametrize("y_on_device", [False, True])
def test_classifier_fit_parity(y_on_device):
    from dbgsom_amd import SomClassifier

    torch = _torch()
    X, y = gi.case_X("digits_clf")
    Xh = np.ascontiguousarray(X, dtype=np.float32)
    Xt = torch.from_numpy(Xh).cuda()
    yt = torch.from_numpy(y).cuda() if y_on_device else y
    host = SomClassifier(**VQ_KW).fit(Xh, y)
    dev = SomClassifier(**VQ_KW).fit(Xt, yt)
    attrs = tuple(a for a in FIT_ATTRS if a != "labels_")   # (the classifier has no labels_)
    _same_fit(dev, host, attrs)
    assert np.array_equal(dev.classes_, host.classes_)
    for attribute in ("label", "probabilities"):
        assert np.array_equal(_node_values(dev, attribute), _node_values(host, attribute)), attribute


def test_entropy_criterion_fit_parity():
    from dbgsom_amd import SomClassifier

    torch = _torch()
    X, y = gi.case_X("digits_entropy")
    kw = gi.EST_KWARGS["digits_entropy"]
    host = SomClassifier(**kw).fit(X, y)
    dev = SomClassifier(**kw).fit(torch.from_numpy(X).cuda(), y)
    _same_fit(dev, host, tuple(a for a in FIT_ATTRS if a != "labels_"))
    for attribute in ("label", "probabilities"):
        assert np.array_equal(_node_values(dev, attribute), _node_values(host, attribute)), attribute


def _same_tree(a, b, attrs, path=()):
    _same_fit(a, b, attrs)
    n_children = 0
    for i, node in enumerate(a.neurons_):
        ca, cb = a.som_.nodes[node].get("som"), b.som_.nodes[node].get("som")
        assert (ca is None) == (cb is None), path + (i,)
        if ca is not None:
            n_children += 1 + _same_tree(ca, cb, attrs, path + (i,))
    return n_children


@pytest.mark.parametrize("supervised", [False, True])
def test_vertical_growth_children_parity(supervised):
    """vertical_growth=True on the blobs of the existing vertical test: the same nodes carry children, and every
    child has the same neurons and prototypes (its Voronoi subset is gathered on the device either way)."""
    from sklearn.datasets import make_blobs

    from dbgsom_amd import SomClassifier, SomVQ

    torch = _torch()
    X, lab = make_blobs(n_samples=4000, n_features=10, centers=7, cluster_std=2.0, random_state=4)
    assert np.array_equal(X, gi.case_X("vertical_blobs")[0])
    kw = gi.EST_KWARGS["vertical_blobs"]
    Xt = torch.from_numpy(X).cuda()
    if supervised:
        host, dev = SomClassifier(**kw).fit(X, lab), SomClassifier(**kw).fit(Xt, lab)
        attrs = tuple(a for a in FIT_ATTRS if a != "labels_")
    else:
        host, dev = SomVQ(**kw).fit(X), SomVQ(**kw).fit(Xt)
        attrs = FIT_ATTRS
    assert _same_tree(dev, host, attrs) >= 1, "the case must grow vertically"


# -- 3. weights ---------------------------------------------------------------------------------------------------
def test_sample_weight_as_a_tensor():
    from dbgsom_amd import SomVQ

    torch = _torch()
    Xh = _digits(np.float32)
    w = np.random.default_rng(5).integers(0, 4, size=Xh.shape[0]).astype(np.float64)
    host = SomVQ(**VQ_KW).fit(Xh, sample_weight=w)
    Xt = torch.from_numpy(Xh).cuda()
    for weights in (w, torch.from_numpy(w).cuda()):
        dev = SomVQ(**VQ_KW).fit(Xt, sample_weight=weights)
        _same_fit(dev, host)


# -- 4. queries on a fitted map -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    from dbgsom_amd import SomClassifier, SomVQ

    X, y = gi.case_X("digits_clf")
    X = X.astype(np.float32)
    vq = SomVQ(**VQ_KW).fit(X)
    clf = SomClassifier(**VQ_KW).fit(X, y)
    for est in (vq, clf):
        est._engine().sc_chunk_rows = 64   # 150 rows: three chunks, the last one short
    return vq, clf


@pytest.fixture(scope="module")
def fitted61():
    """The same two maps on the first 61 features: queries whose rows are no multiple of 16 features long."""
    from dbgsom_amd import SomClassifier, SomVQ

    X, y = gi.case_X("digits_clf")
    X = np.ascontiguousarray(X[:, :61], dtype=np.float32)
    vq = SomVQ(**VQ_KW).fit(X)
    clf = SomClassifier(**VQ_KW).fit(X, y)
    for est in (vq, clf):
        est._engine().sc_chunk_rows = 64
    return vq, clf


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nq", [1, 150])
def test_queries_on_a_tensor_equal_the_host_path(fitted, fitted61, nq, dtype, layout):
    torch = _torch()
    vq, clf = fitted
    rows = np.random.default_rng(nq).choice(1797, nq, replace=False)
    Xh = _digits(dtype)[rows]
    if layout == "d61":
        vq, clf = fitted61
    Xh, Xt = _layout(Xh, layout)
    dev = Xt.device

    def same(t, h, dt):
        assert isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dt, (type(t), dt)
        assert tuple(t.shape) == h.shape
        assert np.array_equal(t.cpu().numpy().view(np.int64), h.view(np.int64))   # (bit for bit, NaN included)

    same(vq.predict(Xt), vq.predict(Xh), torch.int64)
    q_t, q_h = vq.calculate_quantization_error(Xt), vq.calculate_quantization_error(Xh)
    assert isinstance(q_t, float) and q_t == q_h
    same(vq.transform(Xt), vq.transform(Xh), torch.float64)
    same(clf.predict_proba(Xt), clf.predict_proba(Xh), torch.float64)
    p_t, p_h = clf.predict(Xt), clf.predict(Xh)
    assert isinstance(p_t, np.ndarray) and p_t.dtype == p_h.dtype and np.array_equal(p_t, p_h)
    if nq > 1:
        f_t, f_h = vq.topographic_function(Xt), vq.topographic_function(Xh)
        assert all(isinstance(v, np.ndarray) for v in f_t)
        assert np.array_equal(f_t[0], f_h[0]) and np.array_equal(f_t[1], f_h[1])


@pytest.mark.parametrize("layout", ["borrowed", "colslice"])
def test_filtered_query_branch_runs_from_device_rows(layout):
    """A k = 1 query large enough for the filtered search (after lowering filter_min_query_rows): from device rows
    it gives what it gives from host rows, and that is the all-pairs result."""
    from dbgsom_amd.backend import HipBackend

    Xh, Xt = _layout(_digits(np.float32), layout)
    n, d = Xh.shape
    M = 160
    W = Xh[np.random.default_rng(2).choice(n, M, replace=False)].astype(np.float64) + 0.25
    auto, exact = HipBackend(0), HipBackend(0, algorithm="exact")
    auto._set("filter_min_query_rows", 256)
    assert auto.query_filter_applies(n, d, M, 1) and not exact.query_filter_applies(n, d, M, 1)
    d_t, i_t = auto.bmu(W, 1, X=Xt)
    d_h, i_h = auto.bmu(W, 1, X=Xh)
    d_e, i_e = exact.bmu(W, 1, X=Xt)
    assert np.array_equal(i_t.cpu().numpy(), i_h) and np.array_equal(d_t.cpu().numpy(), d_h)
    assert np.array_equal(i_e.cpu().numpy(), i_h) and np.array_equal(d_e.cpu().numpy(), d_h)


# -- 5. nothing of X crosses PCIe ---------------------------------------------------------------------------------
def _moved(be, call):
    before = be.sample_traffic()
    out = call()
    after = be.sample_traffic()
    return out, after["x_upload_bytes"] - before["x_upload_bytes"], after["x_download_bytes"] - before["x_download_bytes"]


def test_sample_traffic_counters():
    from dbgsom_amd import SomClassifier, SomVQ
    from dbgsom_amd.backend import HipBackend

    torch = _torch()
    X, y = gi.case_X("digits_clf")
    Xh = X.astype(np.float32)
    Xt = torch.from_numpy(Xh).cuda()
    n, d = Xh.shape
    be, be_c = HipBackend(0), HipBackend(0)
    assert set(be.traffic()) == {"w_upload_calls", "w_upload_bytes", "w_download_calls", "w_download_bytes",
                                 "w_row_writes", "w_row_reads"}
    vq = SomVQ(backend=be, **VQ_KW)
    _, up, down = _moved(be, lambda: vq.fit(Xt))
    assert up == 0 and down == vq.labels_.nbytes == n * 8
    clf = SomClassifier(backend=be_c, **VQ_KW)
    _, up, down = _moved(be_c, lambda: clf.fit(Xt, y))
    assert up == 0 and down == n * 8          # (the winners the prototypes are labelled from)
    for est, engine, call, returned in ((vq, be, vq.predict, 0), (vq, be, vq.transform, 0),
                                        (clf, be_c, clf.predict_proba, 0), (clf, be_c, clf.predict, n * 8),
                                        # (the mean of the distances is NumPy's, on the host: N x 8 bytes)
                                        (vq, be, vq.calculate_quantization_error, n * 8),
                                        (vq, be, vq.topographic_function, 0)):
        _, up, down = _moved(engine, lambda: call(Xt))
        assert up == 0 and down == returned, call.__name__
    # the same calls on host arrays pay for the rows
    _, up, down = _moved(be, lambda: vq.fit(Xh))
    assert up >= n * d * 4 and down >= n * 8
    for engine, call in ((be, vq.predict), (be, vq.transform), (be_c, clf.predict_proba), (be_c, clf.predict),
                         (be, vq.calculate_quantization_error), (be, vq.topographic_function)):
        _, up, down = _moved(engine, lambda: call(Xh))
        assert up >= n * d * 4, call.__name__


# -- 6. dtypes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["float16", "bfloat16", "int64", "transposed"])
def test_other_dtypes_and_strides_fit_like_their_converted_copy(name):
    from dbgsom_amd import SomVQ

    torch = _torch()
    base = torch.from_numpy(_digits(np.float64)).cuda()     # (integers 0 .. 16: exact in every dtype used here)
    if name == "transposed":
        Xt = base.float().t().contiguous().t()
        assert Xt.stride() == (1, Xt.shape[0])
        like = Xt.contiguous()
    elif name == "int64":
        Xt = base.to(torch.int64)
        like = Xt.double()
    else:
        Xt = base.to(getattr(torch, name))
        like = Xt.float()
    dev = SomVQ(**VQ_KW).fit(Xt)
    host = SomVQ(**VQ_KW).fit(like.cpu().numpy())
    _same_fit(dev, host)
    assert torch.equal(dev.predict(Xt).cpu(), torch.from_numpy(host.predict(like.cpu().numpy())))


# -- 7. refusals ------------------------------------------------------------------------------------------------------
def test_refusals(fitted):
    from dbgsom_amd import SomClassifier, SomVQ
    from dbgsom_amd.backend import HipBackend

    torch = _torch()
    vq, clf = fitted
    Xh = _digits(np.float32)
    Xt = torch.from_numpy(Xh).cuda()
    be = HipBackend(0)
    est = SomVQ(backend=be, **VQ_KW)

    def untouched(call, exc, match):
        before = (be.sample_traffic(), be.traffic(), be.epoch_info())
        with pytest.raises(exc, match=match):
            call()
        after = (be.sample_traffic(), be.traffic(), be.epoch_info())
        assert repr(before) == repr(after)

    for bad, word in ((float("nan"), "NaN"), (float("inf"), "infinity")):
        Xb = Xt.clone()
        Xb[17, 5] = bad
        with pytest.raises(ValueError, match=word):      # (fit: found from the device's column sums)
            SomVQ(**VQ_KW).fit(Xb)
        with pytest.raises(ValueError, match=word):
            SomVQ(**VQ_KW).fit(Xb, sample_weight=np.ones(Xb.shape[0]))
        with pytest.raises(ValueError, match=word):
            vq.predict(Xb[:50])
        with pytest.raises(ValueError, match=word):
            clf.predict_proba(Xb[:50])
    untouched(lambda: est.fit(Xt[:, 0]), ValueError, "Expected 2D array")
    untouched(lambda: est.fit(Xt.reshape(-1, 8, 8)), ValueError, "Expected 2D array")
    untouched(lambda: est.fit(Xt[:3]), ValueError, "minimum of 4 is required")
    with pytest.raises(ValueError, match="X has 61 features, but SomVQ is expecting 64 features"):
        vq.predict(Xt[:, :61])
    with pytest.raises(ValueError, match="X has 61 features, but SomClassifier is expecting 64 features"):
        clf.predict_proba(Xt[:, :61])
    with pytest.raises(ValueError, match="minimum of 1 is required"):
        vq.predict(Xt[:0])
    untouched(lambda: est.fit(Xt.to_sparse()), TypeError, "host array")
    with pytest.raises(TypeError, match="host array"):
        vq.predict(Xt[:20].to_sparse())
    # NaN under missing_values="nan": host arrays only; a complete tensor passes there
    Xn = Xt[:40].clone()
    Xn[3, 3] = float("nan")
    tolerant = SomVQ(missing_values="nan", **VQ_KW).fit(Xt)
    _same_fit(tolerant, vq)
    with pytest.raises(ValueError, match="host array"):
        tolerant.predict(Xn)
    assert torch.equal(tolerant.predict(Xt[:40]).cpu(), torch.from_numpy(vq.predict(Xh[:40])))
    Xf = Xt.clone()
    Xf[3, 3] = float("nan")
    with pytest.raises(ValueError, match="host array"):
        SomVQ(missing_values="nan-fit", **VQ_KW).fit(Xf)
    untouched(lambda: SomVQ(backend=be, sharded_input=True, **VQ_KW).fit(Xt), ValueError, "host array")


def test_vertical_classifier_refuses_tensor_queries():
    from sklearn.datasets import make_blobs

    from dbgsom_amd import SomClassifier

    torch = _torch()
    X, lab = make_blobs(n_samples=4000, n_features=10, centers=7, cluster_std=2.0, random_state=4)
    clf = SomClassifier(**gi.EST_KWARGS["vertical_blobs"]).fit(X, lab)
    Xt = torch.from_numpy(X[:30]).cuda()
    for call in (clf.predict_proba, clf.predict):
        with pytest.raises(ValueError, match="host array"):
            call(Xt)
    assert clf.predict(X[:30]).shape == (30,)
    assert isinstance(clf.transform(Xt), torch.Tensor)     # (the map's own code does not walk the children)


def test_tensor_on_another_gpu_is_refused(fitted):
    from dbgsom_amd import SomVQ

    torch = _torch()
    if torch.cuda.device_count() < 2:
        pytest.skip("one visible GPU")
    vq, _ = fitted
    Xt = torch.from_numpy(_digits(np.float32)).to("cuda:1")
    with pytest.raises(ValueError, match="GPU 1"):
        SomVQ(device=0, **VQ_KW).fit(Xt)
    with pytest.raises(ValueError, match="GPU 1"):
        vq.predict(Xt[:10])
