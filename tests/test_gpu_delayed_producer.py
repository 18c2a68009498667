"""GPU: device tensors whose producer is STILL RUNNING when the method is called (beside tests/test_gpu_device_input.py,
whose tensors are always finished first: its _layout ends in t.cpu()).

The only thing that orders a caller's torch work in front of the context's non-blocking stream is
Backend._producer_done.  Here, on a torch stream P, a tensor that holds a decoy (the true rows rolled by one and halved: a
legal input with another answer) is overwritten with the true values behind a sleep, and the method is called on it
straight away, with an event behind the copy still incomplete.  The result is the host-array call's, bit for bit; what
comes back on the device is read on the null stream, which waits for nothing the context's stream still had to do."""
import numpy as np
import pytest

from tests import golden_inputs as gi
from tests import stream_cases as sc
from tests.test_gpu_device_input import (FIT_ATTRS, VQ_KW, _digits, _node_values, _same_fit, fitted,  # noqa: F401
                                         fitted61)

pytestmark = pytest.mark.gpu

NQ = 150
DELAY_MS = 50.0


def _torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def cycles():
    torch = _torch()
    ms = sc.sleep_ms(torch.cuda.Stream())
    return int(DELAY_MS * sc.SLEEP_C0 / ms)


def _decoy(a):
    return sc.decoy("late", np.ascontiguousarray(a))


class _Late:
    """tensors that hold their decoys now and their true values once the sleep on P is over"""

    def __init__(self, cycles, **arrays):
        torch = _torch()
        self.P = torch.cuda.Stream()
        self.true = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in arrays.items()}
        self.t = {k: torch.from_numpy(_decoy(v)).cuda() for k, v in arrays.items()}
        for k, v in arrays.items():
            assert not np.array_equal(_decoy(v), v), k
        torch.cuda.synchronize()
        self.cycles = cycles

    def call(self, fn):
        """queue the sleep and the copies on P, then fn(tensors) with P current and the copies still pending"""
        torch = _torch()
        with torch.cuda.stream(self.P):
            torch.cuda._sleep(self.cycles)
            for k, t in self.t.items():
                t.copy_(self.true[k])
            ev = torch.cuda.Event()
            ev.record(self.P)
            assert not ev.query(), "delay too short: the producer was done before the call"
            out = fn(**self.t)
        return out


def _host(v):
    torch = _torch()
    if isinstance(v, torch.Tensor):
        return v.cpu().numpy()          # (on the null stream: no wait for the context's stream)
    return v


def _same(got, want, what):
    if isinstance(want, (tuple, list)):
        assert isinstance(got, (tuple, list)) and len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, f"{what}[{i}]")
        return
    g = _host(got)
    if isinstance(want, np.ndarray):
        assert isinstance(g, np.ndarray) and g.dtype == want.dtype and g.shape == want.shape, what
        assert np.array_equal(np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), what
    else:
        assert g == want, what


MIXTURE_KW = dict(bandwidth=8.0, priors="uniform")      # (digits: pixel values 0 .. 16; no fit_mixture on the fixtures)
QUERIES = [
    ("vq", "predict", {}), ("vq", "transform", {}), ("clf", "predict_proba", {}), ("clf", "predict", {}),
    ("vq", "calculate_quantization_error", {}), ("vq", "topographic_function", {}), ("vq", "kneighbors", {}),
    ("vq", "prototype_distances", {}), ("vq", "sample_distortion", {}), ("vq", "prototype_exemplars", {}),
    ("vq", "prototype_density", {}), ("vq", "score_samples", MIXTURE_KW), ("vq", "project", MIXTURE_KW),
    ("vq", "sample_combined_error", {}),
]


@pytest.mark.parametrize("layout", ["borrowed", "d61"])
@pytest.mark.parametrize("est,method,kw", QUERIES, ids=[q[1] for q in QUERIES])
def test_query_on_a_tensor_whose_producer_is_still_running(fitted, fitted61, cycles, est, method, kw, layout):
    vq, clf = fitted61 if layout == "d61" else fitted
    rows = np.random.default_rng(NQ).choice(1797, NQ, replace=False)
    Xh = _digits(np.float32)[rows]
    if layout == "d61":
        Xh = np.ascontiguousarray(Xh[:, :61])
    call = getattr(vq if est == "vq" else clf, method)
    want = call(Xh, **kw)
    late = _Late(cycles, X=Xh)
    got = late.call(lambda X: call(X, **kw))
    _same(got, want, method)


@pytest.mark.parametrize("layout", ["borrowed", "d61"])
def test_fit_on_a_tensor_whose_producer_is_still_running(cycles, layout):
    from dbgsom_amd import SomVQ

    Xh = _digits(np.float32)
    if layout == "d61":
        Xh = np.ascontiguousarray(Xh[:, :61])
    host = SomVQ(**VQ_KW).fit(Xh)
    dev = _Late(cycles, X=Xh).call(lambda X: SomVQ(**VQ_KW).fit(X))
    _same_fit(dev, host)


def test_fit_with_sample_weights_whose_producer_is_still_running(cycles):
    from dbgsom_amd import SomVQ

    torch = _torch()
    Xh = _digits(np.float32)
    w = np.random.default_rng(5).integers(0, 4, size=Xh.shape[0]).astype(np.float64)
    host = SomVQ(**VQ_KW).fit(Xh, sample_weight=w)
    Xt = torch.from_numpy(Xh).cuda()                     # (finished: only the weights are late)
    dev = _Late(cycles, w=w).call(lambda w: SomVQ(**VQ_KW).fit(Xt, sample_weight=w))
    _same_fit(dev, host)


def test_classifier_fit_with_rows_and_labels_whose_producer_is_still_running(cycles):
    from dbgsom_amd import SomClassifier

    X, y = gi.case_X("digits_clf")
    Xh = np.ascontiguousarray(X, dtype=np.float32)
    host = SomClassifier(**VQ_KW).fit(Xh, y)
    dev = _Late(cycles, X=Xh, y=y).call(lambda X, y: SomClassifier(**VQ_KW).fit(X, y))
    attrs = tuple(a for a in FIT_ATTRS if a != "labels_")
    _same_fit(dev, host, attrs)
    assert np.array_equal(dev.classes_, host.classes_)
    for attribute in ("label", "probabilities"):
        assert np.array_equal(_node_values(dev, attribute), _node_values(host, attribute)), attribute


# -- the backend's own queries: nothing of the estimator's validation in front of Backend._producer_done ------------------
BACKEND_QUERIES = [
    ("bmu-k1", lambda be, W, X: be.bmu(W, 1, X=X)), ("bmu-k2", lambda be, W, X: be.bmu(W, 2, X=X)),
    ("distances", lambda be, W, X: be.distances(W, X)), ("kneighbors", lambda be, W, X: be.kneighbors(W, 5, X)),
    ("bmu_manhattan", lambda be, W, X: be.bmu_manhattan(W, 2, X)), ("distances_manhattan", lambda be, W, X: be.distances_manhattan(W, X)),
    ("kneighbors_manhattan", lambda be, W, X: be.kneighbors_manhattan(W, 5, X)),
    ("bmu_cosine", lambda be, W, X: be.bmu_cosine(W, 2, X)), ("distances_cosine", lambda be, W, X: be.distances_cosine(W, X)),
    ("kneighbors_cosine", lambda be, W, X: be.kneighbors_cosine(W, 5, X)),
    ("exemplars", lambda be, W, X: be.exemplars(W, 3, X)), ("sparse_code", lambda be, W, X: be.sparse_code(W, X)),
]


@pytest.fixture(scope="module")
def engine():
    from dbgsom_amd.backend import HipBackend

    return HipBackend(0)


@pytest.mark.parametrize("layout", ["borrowed", "d61"])
@pytest.mark.parametrize("name,call", BACKEND_QUERIES, ids=[q[0] for q in BACKEND_QUERIES])
def test_backend_query_on_a_tensor_whose_producer_is_still_running(engine, cycles, name, call, layout):
    """the estimators look at their rows before they hand them on (a reduction for NaN, read on the host), which waits
    for the producer as a side effect; the backend's queries have Backend._producer_done alone"""
    rows = np.random.default_rng(NQ).choice(1797, NQ, replace=False)
    Xh = _digits(np.float32)[rows]
    if layout == "d61":
        Xh = np.ascontiguousarray(Xh[:, :61])
    W = Xh[np.random.default_rng(2).choice(NQ, 40, replace=False)].astype(np.float64) + 0.25
    want = call(engine, W, Xh)
    late = _Late(cycles, X=Xh)
    # the same call on the finished tensor first: the engine then enters the late call with no staging buffer of the
    # host call left to free (a free waits for the whole device, the producer included, and would hide a missing wait)
    _same(call(engine, W, late.true["X"]), want, name + " (finished tensor)")
    got = late.call(lambda X: call(engine, W, X))
    _same(got, want, name)
