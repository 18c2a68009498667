"""MI355X: every public query path that the two chunked drivers of csrc/engine.hip serve -- the raw-rows driver (rows
with missing entries, ``metric="manhattan"``, ``metric="cosine"``) and the placed-rows driver (the Euclidean distance
matrix, k nearest prototypes, distortion, exemplars, range counts, mixture view and combined error of host rows, rows
in HBM and CSR rows) -- walked as one table: op x form x source x dtype.  Each cell runs twice, in three chunks of
rows and in one, and both runs must give the same bits and move the same bytes.  What the numbers are is checked
elsewhere (tests/test_gpu_missing.py, test_gpu_manhattan.py, test_gpu_cosine.py, test_gpu_prototype_distances.py,
test_gpu_kneighbors.py, test_gpu_distortion.py, test_gpu_exemplars.py, test_gpu_density.py, test_gpu_mixture.py,
test_gpu_combined_error.py); this file pins the drivers' plumbing: chunk offsets, staging buffers, partial last
chunks, per-call results that exist only after the last chunk, row pitches, traffic counters.

N = 131, d = 19, M = 37: d and M are no multiples of 16, and N leaves a partial last chunk under both chunk settings
(64 + 64 + 3 rows for the searches, 50 + 50 + 31 for the matrix and the neighbours, slabs of 16 rows inside them)."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

N, D, M, K, K_BMU = 131, 19, 37, 3, 2
R, V = 2, 3                             # thresholds of the range counts, per-unit values of the mixture view
XPAD, OPAD = 5, 3                       # device rows are D + XPAD elements apart, a device matrix's M + OPAD
SENTINEL = -77.0
CHUNKED = (64, 50, 16)                  # masked_chunk_rows, distances_chunk_rows, kneighbors_slab_rows
ONE_CHUNK = (256, 256, 256)
NP_DTYPE = {"f32": np.float32, "f64": np.float64}
CODE = {"f32": 0, "f64": 1}

SOURCES = {"euclidean": ("host", "device", "csr"), "masked": ("host",), "manhattan": ("host", "device"),
           "cosine": ("host", "device")}
OPS = {"euclidean": ("distances", "kneighbors", "distortion", "exemplars", "exemplars_own", "range_counts", "mixture0",
                     "mixture3", "combined_error"),
       "masked": ("bmu", "distances", "kneighbors"),
       "manhattan": ("bmu", "distances", "kneighbors"), "cosine": ("bmu", "distances", "kneighbors")}
CELLS = [(op, form, source) for form in SOURCES for op in OPS[form] for source in SOURCES[form]]
# chunks of rows that cross PCIe in the chunked run: dense host rows go up chunk by chunk, the three CSR arrays whole
UPLOADS = {"host": 3, "csr": 1, "device": 0}
# what an op sends up once per call beside the rows, counted as sample traffic (one upload call each): H; the
# thresholds; the log-priors and Y; the edges.  And what a whole call brings down: per row, or -- exemplars and range
# counts -- one M-row result after the last chunk.
OPERAND_BYTES = {"distortion": M * M * 8, "range_counts": R * 8, "mixture0": M * 8, "mixture3": M * (1 + V) * 8,
                 "combined_error": M * 8}
DOWN_BYTES = {"bmu": N * K_BMU * 16, "distances": N * M * 8, "kneighbors": N * K * 16, "distortion": N * 16,
              "exemplars": M * K * 16, "exemplars_own": M * K * 16, "range_counts": M * R * 8, "mixture0": N * 16,
              "mixture3": N * (16 + V * 8), "combined_error": N * 24}
SHAPES = {"bmu": [(N, K_BMU)] * 2, "distances": [(N, M)], "kneighbors": [(N, K)] * 2, "distortion": [(N,)] * 2,
          "exemplars": [(M, K)] * 2, "exemplars_own": [(M, K)] * 2, "range_counts": [(M, R)], "mixture0": [(N,)] * 2,
          "mixture3": [(N,), (N,), (N, V)], "combined_error": [(N,), (N, 2)]}


@pytest.fixture(scope="module")
def backend():
    from dbgsom_amd.backend import HipBackend

    be = HipBackend(0)
    yield be
    be.release()


def make_inputs():
    """form, dtype -> (X, W), seeded"""
    rng = np.random.default_rng(131)
    W = rng.normal(size=(M, D))
    out = {}
    for dtype, npdt in NP_DTYPE.items():
        X = (rng.normal(size=(N, D)) * 1.5).astype(npdt)
        Xm = X.copy()
        Xm[rng.random((N, D)) < 0.2] = np.nan
        Xm[np.arange(N), rng.integers(0, D, N)] = X[np.arange(N), 0]            # at least one observed entry per row
        Xs = X * (rng.random((N, D)) < 0.3)
        Xs[57] = 0                                                              # an empty row
        assert not np.isnan(Xm).all(axis=1).any() and 0.15 < np.isnan(Xm).mean() < 0.25
        out["masked", dtype] = (Xm, W)
        out["csr", dtype] = (sp.csr_matrix(Xs), W)
        for form in ("euclidean", "manhattan", "cosine"):
            out[form, dtype] = (X, W)
    for X, _ in out.values():
        if isinstance(X, np.ndarray):
            X.setflags(write=False)
    W.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def inputs():
    """made once, read by every cell"""
    return make_inputs()


def make_operands():
    """what the Euclidean ops take beside X and W, seeded (a generator of their own: the rows above stay as they were)"""
    rng = np.random.default_rng(37)
    H = rng.random((M, M))
    prior = rng.random(M) + 0.1
    ops = {"H": (H + H.T) / 2,                                                  # a symmetric neighbourhood matrix
           "thresholds": np.array([45.0, 75.0]),                                # squared radii that some rows pass and some do not
           "log_prior": np.log(prior / prior.sum()), "c": 0.05, "Y": rng.normal(size=(M, V)),
           "edges": np.stack([np.arange(M), (np.arange(M) + 1) % M], axis=1)}   # a ring over the units
    assert ops["thresholds"].size == R and ops["edges"].shape == (M, 2)
    for a in ops.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ops


@pytest.fixture(scope="module")
def operands():
    """made once, read by every cell"""
    return make_operands()


def _strided(X):
    """the rows on the device, D + XPAD elements apart, NaN between them"""
    import torch

    wide = torch.full((N, D + XPAD), float("nan"), dtype=getattr(torch, str(X.dtype)), device="cuda")
    wide[:, :D] = torch.from_numpy(np.array(X)).cuda()
    view = wide[:, :D]
    assert view.stride(0) == D + XPAD
    return view


def _device_matrix(be, form, dtype, rows, W):
    """the raw *_device call of the distance matrix with rows of the result M + OPAD apart -> (N, M), the spare
    columns checked to hold what they held"""
    import torch

    from dbgsom_amd import _native

    name = "dbgsom_ctx_distances_query_device" if form == "euclidean" else f"dbgsom_ctx_distances_query_{form}_device"
    out = torch.full((N, M + OPAD), SENTINEL, dtype=torch.float64, device="cuda")
    W64 = np.ascontiguousarray(W, dtype=np.float64)
    torch.cuda.synchronize()
    _native.call(name, be._ctx, ctypes.c_void_p(rows.data_ptr()), CODE[dtype], N, D, D + XPAD, W64.ctypes.data, M,
                 ctypes.c_void_p(out.data_ptr()), M + OPAD)
    got = out.cpu().numpy()
    assert (got[:, M:] == SENTINEL).all()
    return got[:, :M]


def _run(be, op, form, source, dtype, X, W, o):
    """one cell -> the arrays of its result, on the host"""
    suffix = "" if form == "euclidean" else "_" + form
    rows = _strided(X) if source == "device" else X
    if op == "distances" and source == "device":
        return (_device_matrix(be, form, dtype, rows, W),)
    if op == "bmu" and form == "masked":
        res = be.bmu_masked(W, K_BMU, rows, want_filled=True)
    elif op == "bmu":
        res = getattr(be, "bmu" + suffix)(W, K_BMU, rows)
    elif op == "distances":
        res = (getattr(be, "distances" + suffix)(W, rows),)
    elif op == "kneighbors":
        res = getattr(be, "kneighbors" + suffix)(W, K, rows)
    elif op == "distortion":
        res = be.neighborhood_energy(W, o["H"], rows)
    elif op in ("exemplars", "exemplars_own"):
        res = be.exemplars(W, K, rows, own_cell=op == "exemplars_own")
    elif op == "range_counts":
        res = (be.range_counts(W, o["thresholds"], rows),)
    elif op in ("mixture0", "mixture3"):
        res = be.mixture(W, o["log_prior"], o["c"], o["Y"] if op == "mixture3" else None, rows)
        res = res[:2] if op == "mixture0" else res                             # (no third result without Y)
    else:
        res = be.combined_error(W, o["edges"], rows)
    return tuple(r.cpu().numpy() if source == "device" else r for r in res)


def _run_with(be, options, *cell):
    """-> (arrays, bytes up, bytes down, upload calls) of one run under the three chunk options"""
    keep = (be.masked_chunk_rows, be.distances_chunk_rows, be.kneighbors_slab_rows)
    try:
        be.masked_chunk_rows, be.distances_chunk_rows, be.kneighbors_slab_rows = options
        before = be.sample_traffic()
        res = _run(be, *cell)
        after = be.sample_traffic()
    finally:
        be.masked_chunk_rows, be.distances_chunk_rows, be.kneighbors_slab_rows = keep
    return res, {k: after[k] - before[k] for k in after}


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("op,form,source", CELLS)
def test_chunked_run_equals_one_chunk_run(backend, inputs, operands, op, form, source, dtype):
    X, W = inputs["csr" if source == "csr" else form, dtype]
    many, moved_many = _run_with(backend, CHUNKED, op, form, source, dtype, X, W, operands)
    one, moved_one = _run_with(backend, ONE_CHUNK, op, form, source, dtype, X, W, operands)
    shapes, down = SHAPES[op], DOWN_BYTES[op]
    operand_bytes = OPERAND_BYTES.get(op, 0)
    operand_calls = 1 if operand_bytes else 0
    if op == "bmu" and form == "masked":
        shapes = shapes + [(N, D)]                                              # the filled rows
        down += N * D * X.dtype.itemsize
    assert [a.shape for a in one] == shapes and len(many) == len(one)
    for a, b in zip(many, one):
        assert np.array_equal(a, b)
    # the same bytes either way (x_upload_calls counts the chunks, so it is the one figure that differs by design)
    for key in ("x_upload_bytes", "x_download_bytes"):
        assert moved_many[key] == moved_one[key]
    if source == "device":                                                      # no row and no result crosses PCIe
        assert moved_one == {"x_upload_bytes": operand_bytes, "x_upload_calls": operand_calls, "x_download_bytes": 0}
    else:
        up = X.data.nbytes + X.indices.nbytes + X.indptr.size * 8 if source == "csr" else X.nbytes
        assert moved_one["x_upload_bytes"] == up + operand_bytes and moved_one["x_download_bytes"] == down
        assert moved_many["x_upload_calls"] == UPLOADS[source] + operand_calls
        assert moved_one["x_upload_calls"] == 1 + operand_calls
