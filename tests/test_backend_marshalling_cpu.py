"""CPU: the C argument list of every query of ``HipBackend``, pinned to a recorded trace.

A recorder -- ``HipBackend`` whose ``_call`` writes the entry point and its arguments down instead of calling the
library -- runs every public query method on every form of X it takes (a host array, an array in HBM, scipy CSR)
and on every input it refuses.  Each call is normalised (scalars as they are, a pointer as the name of the array it
points into) and compared, entry for entry, with ``tests/golden/backend_calls.json``.  That file was recorded with
this module from the backend as it stood BEFORE the row marshalling moved into one helper
(``python -m tests.test_backend_marshalling_cpu <file>`` in a checkout of that commit); it is never recorded from
the code under test, so a swapped ``idx`` / ``dist`` pointer, a lost ``ldx`` or a forgotten wait for X's producer
shows up here, without the built library and without a GPU."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from dbgsom_amd import _native
from dbgsom_amd import backend as backend_mod
from dbgsom_amd.backend import RESIDENT, HipBackend
from tests.test_device_input_cpu import FakeDeviceArray, FakeNamespace

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "backend_calls.json")
D, M, C = 7, 5, 3            # features, prototypes, classes: the smallest shapes at which the branches differ


class Namespace(FakeNamespace):
    """FakeNamespace with ``full``, making arrays of the class below."""

    def empty(self, shape, dtype, device):
        self.calls.append("empty")
        return DeviceArray(np.empty(shape, dtype=dtype), device=device)

    def full(self, shape, value, dtype, device):
        self.calls.append("full")
        return DeviceArray(np.full(shape, value, dtype=dtype), device=device)


NS = Namespace()


class DeviceArray(FakeDeviceArray):
    """FakeDeviceArray of the namespace above.  ``ld``: the row stride an array without rows reports (a torch tensor
    keeps its strides then, NumPy sets them to zero)."""

    def __array_namespace__(self):
        return NS

    def stride(self, i=None):
        st = (self.ld, 1) if self.np.ndim == 2 and self.np.size == 0 else super().stride()
        return st if i is None else st[i]


class Recorder(HipBackend):
    """``HipBackend`` without a library: ``_call`` checks the arguments against the signature and records them.  The
    wait for X's producer is recorded as an event of its own, so that its place in front of the call is pinned."""

    def __init__(self):
        self._ctx = ctypes.c_void_p(1)
        self.device_index = 0
        self._x_traffic = {k: 0 for k in self._X_TRAFFIC}
        self._metric = "euclidean"
        self.events = []

    def __del__(self):
        pass

    def _call(self, fn, *args):
        argtypes = _native.SIGNATURES[fn][1]
        assert len(args) == len(argtypes), (fn, len(args), len(argtypes))
        for a, t in zip(args, argtypes):
            t.from_param(a)            # (raises what the real call would raise)
        self.events.append((fn, args))

    def _producer_done(self, X_dev):
        self.events.append(("_producer_done", (X_dev,)))


# ---------------------------------------------------------------------------------------------------------------
# inputs: float64 C-contiguous W / H / P, int32 coords and edges, canonical CSR with int64 indptr / int32 indices,
# so that the backend hands their own memory to the call and a pointer can be told by its address
def _values(n, d, dtype):
    a = np.random.default_rng(n * 31 + d).standard_normal((n, d))
    a[np.abs(a) < 0.5] = 0.0          # (zeros, so that the CSR form has something to leave out)
    return np.ascontiguousarray(a, dtype=dtype)


def make_X(form, n, dtype, d=D):
    dense = _values(n, d, dtype)
    if form == "host":
        return dense
    if form == "device":              # row stride d + 3
        buf = np.zeros((n, d + 3), dtype=dtype)
        buf[:, :d] = dense
        return DeviceArray(buf[:, :d], ld=d + 3)
    X = sp.csr_matrix(dense)
    X.sort_indices()
    X.indptr, X.indices = X.indptr.astype(np.int64), X.indices.astype(np.int32)
    return X


def make_W(d=D, m=M, dtype=np.float64):
    return np.ascontiguousarray(np.random.default_rng(5).standard_normal((m, d)), dtype=dtype)


H = np.ascontiguousarray(np.random.default_rng(6).random((M, M)))
P = np.ascontiguousarray(np.random.default_rng(7).random((M, C)))
COORDS = np.array([[0, 0], [1, 0], [2, 0], [0, 1], [1, 1]], dtype=np.int32)
EDGES = {0: np.empty((0, 2), dtype=np.int32), 4: np.array([[0, 1], [1, 2], [0, 3], [1, 4]], dtype=np.int32)}
ROWS = [(0, "float64"), (1, "float64"), (9, "float64"), (9, "float32")]
ALL, DENSE, HOST = ("host", "device", "csr"), ("host", "device"), ("host",)
FORMS = {"": ALL, "_manhattan": DENSE, "_cosine": DENSE, "_masked": HOST}


# ---------------------------------------------------------------------------------------------------------------
# the cases: id -> (method name, positional arguments, keyword arguments, loose)
def _cases():
    out = {}

    def add(cid, method, *args, loose=False, **kw):
        assert cid not in out, cid
        out[cid] = (method, args, kw, loose)

    W = make_W()
    for metric, forms in FORMS.items():
        for form in forms:
            for n, dt in ROWS:
                tag = f"{form}/N{n}/{dt}"
                for k in (1, 2):
                    add(f"bmu{metric}/{tag}/k{k}", "bmu" + metric, W, k, X=make_X(form, n, dt))
                    add(f"kneighbors{metric}/{tag}/k{k}", "kneighbors" + metric, W, k, make_X(form, n, dt))
                    if metric == "_masked":
                        add(f"bmu_masked/{tag}/k{k}/filled", "bmu_masked", W, k, make_X(form, n, dt), want_filled=True)
                add(f"distances{metric}/{tag}", "distances" + metric, W, make_X(form, n, dt))
    for form in ALL:
        for n, dt in ROWS:
            tag = f"{form}/N{n}/{dt}"
            add(f"neighborhood_energy/{tag}", "neighborhood_energy", W, H, make_X(form, n, dt))
            for k, own in ((1, False), (2, True)):
                add(f"exemplars/{tag}/k{k}/own{int(own)}", "exemplars", W, k, make_X(form, n, dt), own_cell=own)
            for ne, edges in EDGES.items():
                add(f"combined_error/{tag}/E{ne}", "combined_error", W, edges, make_X(form, n, dt))
    for form in DENSE:
        for n, dt in ROWS:
            tag = f"{form}/N{n}/{dt}"
            for p in (None, P):
                add(f"sparse_code/{tag}/P{int(p is not None)}", "sparse_code", W, make_X(form, n, dt), P=p, max_iter=50)
            for want in (False, True):
                add(f"topographic_function/{tag}/D{int(want)}", "topographic_function", W, make_X(form, n, dt), COORDS,
                    want_distances=want)
        add(f"sparse_code/{form}/resident", "sparse_code", RESIDENT, make_X(form, 9, "float32"))

    # -- the converting paths: only the scalars and the names of the outputs are compared ---------------------
    W32 = make_W(dtype=np.float32)
    for form in ALL:          # float32 prototypes on float32 / float64 rows: the float32-rounding flag
        for dt in ("float32", "float64"):
            add(f"convert/W32/bmu/{form}/{dt}", "bmu", W32, 2, X=make_X(form, 9, dt), loose=True)
            add(f"convert/W32/distances/{form}/{dt}", "distances", W32, make_X(form, 9, dt), loose=True)
            if form != "csr":
                add(f"convert/W32/topographic_function/{form}/{dt}", "topographic_function", W32, make_X(form, 9, dt),
                    COORDS, loose=True)
                add(f"convert/W32/bmu_manhattan/{form}/{dt}", "bmu_manhattan", W32, 1, make_X(form, 9, dt), loose=True)
    add("convert/W32/sparse_code", "sparse_code", W32, make_X("host", 9, "float32"), loose=True)
    Xint = np.arange(9 * D, dtype=np.int64).reshape(9, D) % 5
    Xf = np.asfortranarray(_values(9, D, "float32"))
    Xhalf = _values(9, D, "float16")
    ragged = sp.csr_matrix((np.array([1.0, 2.0, 3.0, 4.0], dtype=np.float32), np.array([4, 1, 1, 6], dtype=np.int32),
                            np.array([0, 3, 3, 4], dtype=np.int32)), shape=(3, D))     # unsorted, with a duplicate
    assert not ragged.has_canonical_format
    for name, X in (("int", Xint), ("fortran", Xf), ("half", Xhalf), ("list", Xint.tolist()), ("ragged_csr", ragged),
                    ("int_csr", sp.csr_matrix(Xint)), ("csc", sp.csc_matrix(_values(9, D, "float32")))):
        sparse = sp.issparse(X)
        add(f"convert/{name}/bmu", "bmu", W, 2, X=X, loose=True)
        if name != "list":        # (the matrix calls read X.shape)
            add(f"convert/{name}/distances", "distances", W, X, loose=True)
            add(f"convert/{name}/exemplars", "exemplars", W, 2, X, loose=True)
            add(f"convert/{name}/combined_error", "combined_error", W, EDGES[4], X, loose=True)
        if not sparse:
            add(f"convert/{name}/bmu_masked", "bmu_masked", W, 1, X, want_filled=True, loose=True)
            add(f"convert/{name}/kneighbors_manhattan", "kneighbors_manhattan", W, 2, X, loose=True)
            add(f"convert/{name}/sparse_code", "sparse_code", W, X, P=P, loose=True)
            add(f"convert/{name}/topographic_function", "topographic_function", W, X, COORDS, loose=True)
    add("convert/edges_int64", "combined_error", W, EDGES[4].astype(np.int64), make_X("host", 9, "float64"), loose=True)
    add("convert/coords_int64", "topographic_function", W, make_X("host", 9, "float64"), COORDS.astype(np.int64),
        loose=True)

    # -- refusals: the exception's type and message ------------------------------------------------------------
    def per_method(tag, X, W=W, only=None, skip=()):
        """One case per query method that takes X's form."""
        form = "csr" if sp.issparse(X) else "device" if isinstance(X, FakeDeviceArray) else "host"
        calls = [("bmu", (W, 2), dict(X=X)), ("distances", (W, X), {}), ("kneighbors", (W, 2, X), {}),
                 ("neighborhood_energy", (W, H, X), {}), ("exemplars", (W, 2, X), {}),
                 ("combined_error", (W, EDGES[4], X), {}),
                 ("sparse_code", (W, X), {}), ("topographic_function", (W, X, COORDS), {})]
        for metric in ("manhattan", "cosine", "masked"):
            calls += [(f"bmu_{metric}", (W, 2, X), {}), (f"distances_{metric}", (W, X), {}),
                      (f"kneighbors_{metric}", (W, 2, X), {})]
        for method, args, kw in calls:
            if only is not None and method not in only or method in skip:
                continue
            if form == "csr" and method in ("sparse_code", "topographic_function"):
                continue              # (the estimators never hand these a sparse matrix)
            add(f"refuse/{tag}/{method}", method, *args, **kw)

    few = ["bmu", "distances", "exemplars", "kneighbors_manhattan", "distances_cosine", "sparse_code",
           "topographic_function"]
    for form in ALL:
        per_method(f"metric_form/{form}", make_X(form, 9, "float64"),
                   only=[f"{op}_{m}" for op in ("bmu", "distances", "kneighbors") for m in ("manhattan", "cosine", "masked")
                         if form not in FORMS["_" + m]])
        per_method(f"features/{form}", make_X(form, 9, "float64"), W=make_W(d=D + 1))
        per_method(f"W_1d/{form}", make_X(form, 9, "float64"), W=make_W()[0], only=few + ["kneighbors", "bmu_masked"])
    per_method("X_1d/host", _values(9, D, "float64")[0], only=few + ["kneighbors", "bmu_masked"])
    per_method("X_1d/device", DeviceArray(_values(9, D, "float64")[0]), only=few + ["kneighbors", "bmu_masked"])
    per_method("X_3d/host", _values(9, D, "float64").reshape(3, 3, D), only=few)
    wide = np.zeros((9, D + 3), dtype=np.float16)
    per_method("device_dtype", DeviceArray(wide[:, :D], half="float16"))
    per_method("device_dtype_bf16", DeviceArray(wide[:, :D], half="bfloat16"), only=few)
    per_method("device_dtype_int", DeviceArray(np.zeros((9, D), dtype=np.int64)), only=few)
    per_method("device_dtype/N0", DeviceArray(wide[:0, :D], half="float16", ld=D + 3))
    per_method("device_column_stride", DeviceArray(np.asfortranarray(_values(9, D, "float64"))), only=few)
    per_method("device_row_stride", DeviceArray(np.broadcast_to(_values(1, D, "float64"), (9, D))), only=few)
    per_method("device_other_gpu", DeviceArray(_values(9, D, "float64"), index=1), only=few)
    per_method("csr_empty", make_X("csr", 0, "float64"), only=["bmu"])
    # two refusals at once: which one is raised
    per_method("device_dtype+features", DeviceArray(wide[:, :D], half="float16"), W=make_W(d=D + 1))
    per_method("device_other_gpu+features/N0", DeviceArray(_values(0, D, "float64"), index=1, ld=D), W=make_W(d=D + 1),
               only=few)
    per_method("csr_empty+features", make_X("csr", 0, "float64"), W=make_W(d=D + 1))
    per_method("metric_form+features/csr", make_X("csr", 9, "float64"), W=make_W(d=D + 1),
               only=["bmu_manhattan", "distances_cosine", "kneighbors_masked"])
    per_method("metric_form+features/device", make_X("device", 9, "float64"), W=make_W(d=D + 1),
               only=["bmu_masked", "distances_masked", "kneighbors_masked"])
    for form in ALL:
        for metric in FORMS:
            if form in FORMS[metric]:
                for k in (0, M + 1):
                    add(f"refuse/k{k}/kneighbors{metric}/{form}", "kneighbors" + metric, W, k, make_X(form, 9, "float64"))
                add(f"refuse/k0+features/kneighbors{metric}/{form}", "kneighbors" + metric, make_W(d=D + 1), 0,
                    make_X(form, 9, "float64"))
        add(f"refuse/k33/kneighbors/{form}", "kneighbors", make_W(m=40), 33, make_X(form, 9, "float64"))
        for k in (0, _native.MAX_NEIGHBORS + 1):
            add(f"refuse/k{k}/exemplars/{form}", "exemplars", W, k, make_X(form, 9, "float64"))
            add(f"refuse/k{k}/exemplars/{form}/N0", "exemplars", W, k, make_X(form, 0, "float64"))
        add(f"refuse/H_shape/{form}", "neighborhood_energy", W, H[:, :4], make_X(form, 9, "float64"))
        add(f"refuse/H_shape/{form}/N0", "neighborhood_energy", W, H[:4], make_X(form, 0, "float64"))
        add(f"refuse/edges_float/{form}", "combined_error", W, EDGES[4].astype(np.float64), make_X(form, 9, "float64"))
        add(f"refuse/edges_shape/{form}", "combined_error", W, EDGES[4].reshape(-1), make_X(form, 9, "float64"))
        add(f"refuse/edges_range/{form}", "combined_error", W, EDGES[4] + 1, make_X(form, 9, "float64"))
        add(f"refuse/one_prototype/{form}", "combined_error", make_W(m=1), EDGES[0], make_X(form, 9, "float64"))
    bad = DeviceArray(wide[:, :D], half="float16")
    for form in DENSE:
        add(f"refuse/P_rows/{form}", "sparse_code", W, make_X(form, 9, "float64"), P=P[:4])
        add(f"refuse/P_1d/{form}", "sparse_code", W, make_X(form, 9, "float64"), P=P[:, 0])
        add(f"refuse/coords_rows/{form}", "topographic_function", W, make_X(form, 9, "float64"), COORDS[:4])
        add(f"refuse/resident_features/{form}", "sparse_code", RESIDENT, make_X(form, 9, "float64", d=D + 1))
    add("refuse/device_dtype+k0/kneighbors", "kneighbors", W, 0, bad)
    add("refuse/device_dtype+k0/kneighbors_manhattan", "kneighbors_manhattan", W, 0, bad)
    add("refuse/device_dtype+k0/exemplars", "exemplars", W, 0, bad)
    add("refuse/device_dtype+H_shape", "neighborhood_energy", W, H[:4], bad)
    add("refuse/device_dtype+edges_range", "combined_error", W, EDGES[4] + 1, bad)
    add("refuse/device_dtype+W_1d/sparse_code", "sparse_code", make_W()[0], bad)
    add("refuse/device_dtype+P_rows/sparse_code", "sparse_code", W, bad, P=P[:4])
    add("refuse/device_dtype+coords_rows", "topographic_function", W, bad, COORDS[:4])
    add("refuse/X_1d+W_1d/sparse_code", "sparse_code", make_W()[0], _values(9, D, "float64")[0])
    for dt in ("bf16", np.dtype(np.float32), np.dtype(np.float64), np.dtype(np.int32), np.dtype(np.float16)):
        add(f"refuse/_x_dtype_code/{dt}", "_x_dtype_code", dt)
    return out


CASES = _cases()


# ---------------------------------------------------------------------------------------------------------------
def _address(a):
    """-> (first byte, bytes) of the memory a NumPy array lives in, its base's when it is a view"""
    while isinstance(a.base, np.ndarray):
        a = a.base
    return a.ctypes.data, a.nbytes


def _arrays_of(X):
    if isinstance(X, FakeDeviceArray):
        return {"X": X.np}
    if sp.issparse(X):
        return {"indptr": X.indptr, "indices": X.indices, "data": X.data}
    return {"X": X} if isinstance(X, np.ndarray) else {}


def _named_inputs(method, args, kw):
    names = {"bmu": ("W", "k", "X"), "distances": ("W", "X"), "kneighbors": ("W", "k", "X"),
             "neighborhood_energy": ("W", "H", "X"), "exemplars": ("W", "k", "X"),
             "combined_error": ("W", "edges", "X"), "sparse_code": ("W", "X", "P"),
             "topographic_function": ("W", "X", "coords")}[re.sub("_(manhattan|cosine|masked)$", "", method)]
    given = dict(zip(names, args), **kw)
    named = {}
    for name, v in given.items():
        if name == "X":
            named.update(_arrays_of(v))
        elif isinstance(v, np.ndarray):
            named[name] = v
    return named, given.get("X")


def _describe(r, called):
    if r is None:
        return None
    kind, a = ("dev", r.np) if isinstance(r, FakeDeviceArray) else ("np", r)
    out = f"{kind} {'x'.join(map(str, a.shape))} {a.dtype}"
    if not called and a.size:      # (made without a launch: what it was filled with)
        values = np.unique(a)
        out += " of " + (repr(float(values[0])) if values.size == 1 else "mixed values")
    return out


def run_case(cid):
    method, args, kw, loose = CASES[cid]
    if method == "_x_dtype_code":
        try:
            return {"returns": backend_mod._x_dtype_code(*args)}
        except Exception as e:  # noqa: BLE001
            return {"raises": [type(e).__name__, str(e)]}
    rec = Recorder()
    if args[0] is RESIDENT:        # what a loaded context would answer
        rec._loaded, rec._d, rec._get = True, D, lambda name: {"prototypes": M}[name]
    named, X = _named_inputs(method, args, kw)
    del NS.calls[:]
    entry = {}
    try:
        result = getattr(rec, method)(*args, **kw)
    except Exception as e:  # noqa: BLE001
        entry["raises"] = [type(e).__name__, str(e)]
        result = ()
    if not isinstance(result, tuple):
        result = (result,)
    called = any(fn != "_producer_done" for fn, _ in rec.events)
    for i, r in enumerate(result):
        if r is not None:
            named[f"ret{i}"] = r.np if isinstance(r, FakeDeviceArray) else r
    spans = [(name,) + _address(a) for name, a in named.items()]

    def pointer(p):
        if isinstance(p, ctypes.c_void_p):
            p = p.value
        if p is None:
            return "null"
        for name, first, size in spans:
            if p == first or first <= p < first + size:
                return name if not loose or name.startswith("ret") else "in"
        return "in" if loose else "buf"

    calls = []
    for fn, a in rec.events:
        if fn == "_producer_done":
            calls.append(f"_producer_done({'X' if a[0] is X else 'other'})")
            continue
        argtypes = _native.SIGNATURES[fn][1]
        assert a[0] is rec._ctx
        norm = ["ctx"] + [pointer(v) if t is ctypes.c_void_p else repr(float(v) if isinstance(v, float) else int(v))
                          for v, t in zip(a[1:], argtypes[1:])]
        calls.append(f"{fn}({', '.join(norm)})")
    if calls or "raises" not in entry:
        entry["calls"] = calls
    if "raises" not in entry:
        entry["returns"] = [_describe(r, called) for r in result]
    if NS.calls:
        entry["namespace"] = list(NS.calls)
    return entry


def record(path):
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(cid)}: {json.dumps(run_case(cid), separators=(',', ':'))}"
                                   for cid in CASES) + "\n}\n")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_cases_are_the_recorded_ones(golden):
    assert list(golden) == list(CASES)


@pytest.mark.parametrize("group", sorted({cid.split("/")[0] for cid in CASES} - {"refuse", "convert"}) + ["refuse", "convert"])
def test_calls_match_the_recorded_trace(golden, group):
    wrong = {}
    for cid in CASES:
        if cid.split("/")[0] == group:
            got = json.loads(json.dumps(run_case(cid)))
            if got != golden[cid]:
                wrong[cid] = (got, golden[cid])
    assert not wrong, "\n".join(f"{cid}\n   now      {g}\n   recorded {e}" for cid, (g, e) in list(wrong.items())[:8])


def test_the_recorded_trace_holds_the_refusals_and_the_empty_input_rules(golden):
    """The recorded trace itself holds what it is there to pin: every refusal with its text and without a call, and
    what each query does with rows that are none."""
    for cid, entry in golden.items():
        if cid.startswith("refuse/") and "_x_dtype_code/" not in cid and "N0" not in cid:
            assert "raises" in entry and "calls" not in entry, cid
    texts = {tuple(e["raises"]) for e in golden.values() if "raises" in e}
    for expected in (("TypeError", "the Manhattan calls take dense rows"), ("TypeError", "the cosine calls take dense rows"),
                     ("TypeError", "the masked calls take dense rows"), ("TypeError", "the masked calls take host rows"),
                     ("ValueError", "prototype / sample feature mismatch"),
                     ("ValueError", "device rows must be a 2-D array of float32 / float64"),
                     ("ValueError", "device rows need unit column stride and a row stride of at least their length"),
                     ("ValueError", "the rows live on GPU 1, this backend runs on GPU 0"),
                     ("ValueError", "X must be a non-empty 2-D array"),
                     ("ValueError", "samples must be float32 or float64, got int32")):
        assert expected in texts, expected
    for op in ("distances", "kneighbors/", "neighborhood_energy", "combined_error"):     # empty: no call
        empties = [e for cid, e in golden.items() if cid.startswith(op) and "/N0/" in cid]
        assert empties and all(e["calls"] == [] for e in empties), op
    for cid, e in golden.items():
        if cid.startswith("exemplars/") and "/N0/" in cid:
            assert e["calls"] == [] and [r.split(" of ")[1] for r in e["returns"]] == ["inf", "-1.0"], cid
            assert e.get("namespace", ["full", "full"]) == ["full", "full"], cid
        if cid.startswith(("bmu/host/N0", "bmu/device/N0", "bmu_manhattan/host/N0", "sparse_code/host/N0")):
            assert len(e["calls"]) - e["calls"][0].startswith("_producer_done") == 1, cid


if __name__ == "__main__":
    record(sys.argv[1])
    print(f"{len(CASES)} cases -> {sys.argv[1]}")
