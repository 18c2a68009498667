"""The stream contract of include/dbgsom_hip.h -- "device-level calls only ENQUEUE work on `stream`; the caller
synchronises" -- as something a test can fail on (tests/test_gpu_streams.py, tests/test_streams_cpu.py; DESIGN.md
6.5).  Helpers and tables only, no tests in here.

On the legacy null stream, where every other raw-call test runs, a launch that forgot its stream argument, a clear
queued on stream 0 or a helper that waits where it should only queue all give the bits of correct code.  Here an
entry runs on a NON-BLOCKING stream the library itself made (the stream of a context: production's flags and
priority) behind a delay, and everything it reads and writes is put in place on that stream, behind the same delay:

  before the delay      every input's live buffer holds a DECOY (a legal input that gives another answer), the
                        workspace zeros, every output buffer TAIL
  on the stream S       sleep | true inputs -> live buffers | workspace <- 0xFF | output bodies <- fill | pre |
                        event `before` | THE ENTRY | clones of the outputs | event `after`
  on the host           the time of the entry's return and before.query() straight after it

A read issued on another stream sees the decoy; a clear or a write issued on another stream lands in front of the
fills and is overwritten; a wait the header does not promise shows as before.query() == True on return.

Decoys: float inputs are the true rows rolled by one and halved (finite where the rolled input is, the same shape
and type); integer inputs that only need each element in a range (winners, owners, source lists) are rolled by one
position; integer inputs that shape memory access (FIXED) keep the true values -- a mis-ordered read has to give a
wrong ANSWER, never a fault."""
import ctypes
import functools
import re
import time

import numpy as np

from tests import device_abi as da
from tests import workspace_cases as wc

D_MS = 100.0              # the delay in front of every delayed run (DESIGN.md 6.5 holds the measured call times)
MARGIN = 20               # D >= MARGIN x the host time an enqueue-only entry takes to return on the null stream
SLEEP_C0 = 20_000_000     # cycles of the calibration sleep
MAX_STREAMS = 3           # streams of our own that are ever open

# integer inputs that shape memory access: their live buffers hold the true values throughout
FIXED = ("indptr", "indices", "edges", "xy", "order", "seg_start", "idx2")
# arrays a case keeps beside its inputs for its reference; no entry is handed their address
HOST_ONLY = {"dense": "the dense image of the CSR rows, read by the reference only"}

# entries that wait for the stream: entry -> the header's own words
BLOCKS = {
    "dbgsom_topofn": "The call is blocking (it reads back the kernels' status word)",
    "dbgsom_geodesics": "Blocking: the status word is read back.",
    "dbgsom_edge_lengths": "An index outside [0, M) reads nothing, leaves NaN and is DBGSOM_ERANGE. Blocking.",
    "dbgsom_combined_error_rows": "An index outside [0, M) other than -1 reads nothing, leaves NaN and is DBGSOM_ERANGE. Blocking.",
}

# decoyed inputs whose decoy cannot change an output bit: (entry, case label or None for every case, input) -> why
UNOBSERVABLE = {
    ("dbgsom_weighted_column_sums", "N513-d37-f64", "mean"): "this case passes NULL for the mean (plain weighted sums)",
}

# entries of the header that take a stream and run behind no delay: entry -> the reason (never "not built yet").  An entry
# that is neither here nor in a case, a `pre` step or a sequence fails tests/test_streams_cpu.py.
EXEMPT = {}
# entries reached as the `pre` step of a case, on the same stream and behind the same delay
PRE_STEPS = {"dbgsom_topk_cols_init": "dbgsom_topk_cols"}


def stream_entries(header_text):
    """-> {entry: number of parameters} of every prototype of the header whose last parameter is `void *stream`"""
    out = {}
    for name, params in re.findall(r"^int (dbgsom_\w+)\(([^;{]*?)\);", header_text, re.M | re.S):
        params = [p.strip() for p in params.replace("\n", " ").split(",")]
        if params[-1] == "void *stream":
            out[name] = len(params)
    return out


def cases():
    """(size function, case index) of every record that goes through workspace_cases.run_case"""
    return wc.all_cases()


def covered():
    """-> {entry: where}: the entries a case of this file runs"""
    out = {wc.records()[name].entry: "case" for name, _ in cases()}
    out.update({pre: f"pre of {entry}" for pre, entry in PRE_STEPS.items()})
    out.update({entry: f"step '{step}' of the filtered sequence" for step, entry in SEQUENCE_STEPS.items()})
    out.update({entry: f"step '{step}' of the anchored sequence" for step, entry in ANCHORED_STEPS.items() if entry not in out})
    out.update({entry: "case" for entry in plain_records()})
    return out


def live_inputs(case):
    """-> {name: host array} of the inputs an entry is handed, in the case's own order"""
    return {k: v for k, v in case.inputs().items() if k not in HOST_ONLY}


def decoy(name, v):
    """a legal input of v's shape and type that is not v (FIXED: v itself)"""
    v = np.ascontiguousarray(v)
    if name in FIXED:
        return v.copy()
    if v.dtype.kind == "f":
        return np.ascontiguousarray(np.roll(v, 1, axis=0) * v.dtype.type(0.5))
    if v.dtype.kind == "i":
        return np.ascontiguousarray(np.roll(v.reshape(-1), 1).reshape(v.shape))
    raise TypeError(f"no decoy for input '{name}' of type {v.dtype}")


def unobservable(rec, case, name):
    return UNOBSERVABLE.get((rec.entry, case.label, name)) or UNOBSERVABLE.get((rec.entry, None, name))


# ---- the rig (GPU) --------------------------------------------------------------------------------------------------
def sleep_ms(S):
    """time one sleep of SLEEP_C0 cycles on stream S with two events (the second of two sleeps: the first one loads the
    kernel) -> milliseconds"""
    import torch

    ms = 0.0
    for _ in range(2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(S):
            a.record(S)
            torch.cuda._sleep(SLEEP_C0)
            b.record(S)
        S.synchronize()
        ms = a.elapsed_time(b)
    assert ms > 0.0, "the calibration sleep took no time"
    return ms


class Rig:
    """up to MAX_STREAMS non-blocking streams, each the stream of a context of its own (dbgsom_ctx_create, then
    dbgsom_ctx_stream: production's stream), wrapped for torch; the calibrated sleep"""

    def __init__(self, nat):
        self.nat, self.ctxs, self.streams = nat, [], []
        self.cycles_per_ms = None

    def stream(self, i=0):
        import torch

        assert 0 <= i < MAX_STREAMS
        while len(self.streams) <= i:
            ctx, raw = ctypes.c_void_p(), ctypes.c_void_p()
            self.nat.call("dbgsom_ctx_create", 0, ctypes.byref(ctx))
            self.ctxs.append(ctx)
            self.nat.call("dbgsom_ctx_stream", ctx, ctypes.byref(raw))
            assert raw.value, "the context's stream is the null stream"
            self.streams.append(torch.cuda.ExternalStream(raw.value, device=torch.device("cuda", 0)))
        return self.streams[i]

    def close(self):
        import torch

        torch.cuda.synchronize()
        self.streams = []
        while self.ctxs:
            self.nat.call("dbgsom_ctx_destroy", self.ctxs.pop())

    def calibrate(self):
        """-> the milliseconds one sleep of SLEEP_C0 cycles takes on the stream"""
        ms = sleep_ms(self.stream(0))
        self.cycles_per_ms = SLEEP_C0 / ms
        return ms

    def cycles(self, ms=D_MS):
        assert self.cycles_per_ms, "calibrate() first"
        return int(ms * self.cycles_per_ms)


_DECOYS = {}


def _decoys(case):
    """the device copies of a case's decoys, made once and read only"""
    if case not in _DECOYS:
        _DECOYS[case] = {k: da.dev(decoy(k, v) if v.size else np.zeros(1, dtype=v.dtype))
                         for k, v in live_inputs(case).items()}
    return _DECOYS[case]


class Pending:
    """a run that has been queued: everything it touches stays alive in here until finish()"""


def prepare(nat, rec, case):
    """allocate what one run touches, on the null stream: live buffers holding the decoys, a workspace of zeros, output
    buffers of TAIL.  The caller synchronises the device before launch()."""
    import torch

    r = Pending()
    r.nat, r.rec, r.case = nat, rec, case
    r.live = {k: t.clone() for k, t in _decoys(case).items()}
    r.n = rec.nbytes(nat.load(), case)
    r.ws_t, r.ws = da.workspace(r.n)
    r.bufs = {name: torch.full((cnt + 2 * wc.PAD,), wc.TAIL[dtype], dtype=getattr(torch, dtype), device="cuda")
              for name, (cnt, dtype, fill) in case.outputs.items()}
    r.p = {k: t.data_ptr() for k, t in r.live.items()}
    for name, t in r.bufs.items():
        r.p[name] = t.data_ptr() + wc.PAD * t.element_size()
    wc.staged(case)
    return r


def launch(r, S=None, cycles=0, keep_decoy=()):
    """queue a prepared run: S = None is the null stream (no delay: the warm-up and the bits to compare with);
    keep_decoy: the inputs whose live buffers are NOT overwritten with the true values (the sensitivity control).
    Nothing of the run is read before finish()."""
    import torch

    nat, rec, case, p = r.nat, r.rec, r.case, r.p
    true = wc.staged(case).t
    r.S = S
    stream = torch.cuda.current_stream() if S is None else S
    with torch.cuda.stream(stream):
        r.t_sleep = time.perf_counter()
        if cycles:
            torch.cuda._sleep(cycles)
        for k, t in r.live.items():
            if k not in keep_decoy:
                t.copy_(true[k])
        r.ws_t.fill_(0xFF)
        for name, (cnt, dtype, fill) in case.outputs.items():
            r.bufs[name][wc.PAD:wc.PAD + cnt] = fill
        if case.pre is not None:
            case.pre(nat, p)                       # (launches on da.stream(): the current stream, this one)
        r.before = torch.cuda.Event(enable_timing=True)
        r.before.record(stream)
        args = case.args(p, r.ws, r.n)
        entry = getattr(nat.load(), rec.entry)
        r.t_call = time.perf_counter()
        r.rc = entry(*args, ctypes.c_void_p(stream.cuda_stream))
        r.t_ret = time.perf_counter()
        r.done_on_return = r.before.query()
        r.clones = {name: t.clone() for name, t in r.bufs.items()}
        r.inout = {name: r.live[name].clone() for name in getattr(case, "inout", ())}      # arguments written in place
        r.after = torch.cuda.Event(enable_timing=True)
        r.after.record(stream)
    return r


def enqueue(nat, rec, case, S=None, cycles=0, keep_decoy=()):
    """prepare, synchronise the device, launch"""
    import torch

    r = prepare(nat, rec, case)
    torch.cuda.synchronize()
    return launch(r, S, cycles, keep_decoy)


def finish(r):
    """wait for the run's stream -> {name: host array} from the clones queued straight behind the entry; the sentinels
    around every output are checked"""
    import torch

    try:
        (torch.cuda.current_stream() if r.S is None else r.S).synchronize()
        torch.cuda.synchronize()
    except RuntimeError as e:                 # a fault of the device: nothing more is started on it in this session
        import pytest

        pytest.exit(f"{r.rec.entry} {r.case.label}: the device faulted ({e})", returncode=3)
    out = {}
    for name, (n, dtype, fill) in r.case.outputs.items():
        h, late = r.clones[name].cpu().numpy(), r.bufs[name].cpu().numpy()
        tail = np.full(wc.PAD, np.array(wc.TAIL[dtype], dtype=h.dtype))
        for image in (h, late):
            assert wc.same_bits(image[:wc.PAD], tail) and wc.same_bits(image[wc.PAD + n:], tail), \
                f"{r.rec.entry} {r.case.label}: a write outside output '{name}'"
        assert wc.same_bits(h, late), f"{r.rec.entry} {r.case.label}: output '{name}' changed behind the entry's clone"
        out[name] = h[wc.PAD:wc.PAD + n].copy()
    for name, t in r.inout.items():
        out[name] = t.cpu().numpy().reshape(-1)
        assert wc.same_bits(out[name], r.live[name].cpu().numpy().reshape(-1)), \
            f"{r.rec.entry} {r.case.label}: '{name}' changed behind the entry's clone"
    return out


def check_delay(r, what=""):
    """the delay checks itself: the host was done with its part (the entry's return; a blocking entry's call) in the
    first half of the delay, and the entry waited exactly where the header says it does"""
    blocking = r.rec.entry in BLOCKS
    host_ms = ((r.t_call if blocking else r.t_ret) - r.t_sleep) * 1e3
    assert host_ms < D_MS / 2, f"{r.rec.entry} {r.case.label}{what}: delay too short ({host_ms:.2f} ms of host work, D = {D_MS} ms)"
    if blocking:
        assert r.done_on_return, f"{r.rec.entry} {r.case.label}{what}: documented as blocking, returned with its stream still busy"
    else:
        assert not r.done_on_return, \
            f"{r.rec.entry} {r.case.label}{what}: waited for its stream (took {(r.t_ret - r.t_call) * 1e3:.2f} ms to return); " \
            "the header promises it only enqueues"


# ---- the filtered family: one sequence on one workspace (the workspace with a contents contract) -----------------------
# step -> the entry it calls; the anchored forms and their readers have a sequence of their own further down
SEQUENCE_SHAPES = (3, 2)             # rows of filter_device.RAW_SHAPES: (1000, 48, 300) and (129, 16, 129)
SEQUENCE_STEPS = {
    "norms": "dbgsom_row_sqnorms", "prepare": "dbgsom_filter_prepare", "search": "dbgsom_bmu_filtered",
    "counts_async": "dbgsom_bmu_filtered_counts_async", "counts": "dbgsom_bmu_filtered_counts",
    "gaps": "dbgsom_bmu_filtered_gaps", "lists": "dbgsom_bmu_filtered_lists",
    "refine_counts": "dbgsom_bmu_filtered_refine_counts",
}
READERS = ("counts", "gaps", "lists", "refine_counts")          # the blocking ones, in the order they are called
BLOCKS.update({
    "dbgsom_bmu_filtered_counts": "Synchronises the stream.",
    "dbgsom_bmu_filtered_gaps": "Synchronises the stream.",
    "dbgsom_bmu_filtered_lists": "Synchronises the stream.",
    "dbgsom_bmu_filtered_refine_counts": "synchronises the stream",
})
SEQUENCE_FIXED = {"prev": "any seed gives the exact result, so a decoy could not be seen; the true seeds stay",
                  "order": "shapes memory access"}


def search_calls():
    """(label, hinted, flags) of the dbgsom_bmu_filtered calls of the sequence, the last one with DBGSOM_PRUNE (the gap
    table) and DBGSOM_REFINE (its counters)"""
    from tests import filter_device as fd

    return (("stateless", False, 0), ("stateless-prune", False, fd.PRUNE), ("hinted", True, 0),
            ("hinted-prune", True, fd.PRUNE), ("prune-refine", False, fd.PRUNE | fd.REFINE))


class FilteredInputs:
    """host inputs, decoys and the chain reference of one shape, and their device copies: made once, read only"""

    def __init__(self, si):
        from oracle import som_oracle as o
        from tests import filter_device as fd

        self.si = si
        self.N, self.d, self.M = fd.RAW_SHAPES[si]
        X, W = fd.raw_data(si, "f32")
        self.ref_dist, self.ref_idx = o.bmu_chain(X, W, 1)
        prev, order = fd.raw_seeds("random", X, W, self.ref_idx, ("stream", si))
        self.host = dict(X=np.ascontiguousarray(X), W=np.ascontiguousarray(W), prev=prev, order=order)
        self.decoys = {k: (v.copy() if k in SEQUENCE_FIXED else decoy(k, v)) for k, v in self.host.items()}
        self._dev = None

    def dev(self):
        if self._dev is None:
            self._dev = ({k: da.dev(v) for k, v in self.host.items()}, {k: da.dev(v) for k, v in self.decoys.items()})
        return self._dev


class FilteredRun:
    """one run of the sequence.  prepare (null stream) -> the caller synchronises -> launch_searches (enqueue-only
    steps) -> read (the blocking readers, each behind a delay of its own) -> finish."""

    def __init__(self, nat, inp):
        import torch

        self.nat, self.inp = nat, inp
        N, d, M = inp.N, inp.d, inp.M
        lib = nat.load()
        true, decoys = inp.dev()
        self.live = {k: t.clone() for k, t in decoys.items()}
        self.xx = torch.full((N,), -1.0, dtype=torch.float64, device="cuda")
        self.ww = torch.full((M,), -1.0, dtype=torch.float64, device="cuda")
        self.pbytes = int(lib.dbgsom_filter_planes_bytes(N, d))
        self.planes = torch.zeros(self.pbytes + 512, dtype=torch.uint8, device="cuda")
        self.pptr = (self.planes.data_ptr() + 255) // 256 * 256
        self.n = int(lib.dbgsom_bmu_filtered_workspace_bytes(N, d, M))
        self.ws_t = torch.full((self.n + 256,), 0xFF, dtype=torch.uint8, device="cuda")   # zero-filled once: on the stream
        self.ws = (self.ws_t.data_ptr() + 255) // 256 * 256
        self.idx = [torch.full((N + 2 * wc.PAD,), wc.TAIL["int64"], dtype=torch.int64, device="cuda") for _ in search_calls()]
        self.dist = [torch.full((N + 2 * wc.PAD,), wc.TAIL["float64"], dtype=torch.float64, device="cuda") for _ in search_calls()]
        self.nb = (N + 127) // 128
        self.counts_async = torch.full((self.nb,), -1, dtype=torch.int32).pin_memory()
        self.host_out = {"counts": np.full(self.nb, 0xFFFFFFFF, dtype=np.uint32), "gaps": np.full((M, M), np.nan, dtype=np.float32),
                         "lists": np.full((self.nb, M), 0xFFFF, dtype=np.uint16), "refine_counts": np.zeros(4, dtype=np.uint64)}
        self.events = {}                       # (step, label) -> the events recorded on the stream around the call
        self.steps = []                        # (step, label, status, before.query() on return, ms from the sleep to call / return)

    def _stream(self, S):
        import torch

        return torch.cuda.current_stream() if S is None else S

    def launch_searches(self, S=None, cycles=0, keep_decoy=(), only=None):
        import torch

        lib, inp = self.nat.load(), self.inp
        N, d, M = inp.N, inp.d, inp.M
        true = inp.dev()[0]
        self.S = S
        stream = self._stream(S)
        s = ctypes.c_void_p(stream.cuda_stream)
        with torch.cuda.stream(stream):
            t0 = time.perf_counter()
            if cycles:
                torch.cuda._sleep(cycles)
            for k, t in self.live.items():
                if k not in keep_decoy:
                    t.copy_(true[k])
            self.ws_t.zero_()
            self.planes.fill_(0x7f)
            self.xx.fill_(float("nan"))
            self.ww.fill_(float("nan"))
            for i in range(len(self.idx)):
                self.idx[i][wc.PAD:wc.PAD + N] = -7
                self.dist[i][wc.PAD:wc.PAD + N] = float("nan")

            def step(name, label, fn, *args):
                ev, behind = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev.record(stream)
                t1 = time.perf_counter()
                rc = fn(*args, s)
                t2 = time.perf_counter()
                done = ev.query()
                behind.record(stream)
                self.steps.append((name, label, rc, done, (t1 - t0) * 1e3, (t2 - t0) * 1e3))
                self.events[(name, label)] = (ev, behind)

            x = self.live["X"].data_ptr()
            step("norms", "X", lib.dbgsom_row_sqnorms, x, da.F32, N, d, d, self.xx.data_ptr())
            step("norms", "W", lib.dbgsom_row_sqnorms, self.live["W"].data_ptr(), da.F64, M, d, d, self.ww.data_ptr())
            step("prepare", "X", lib.dbgsom_filter_prepare, x, da.F32, N, d, d, self.pptr, self.pbytes)
            for i, (label, hinted, flags) in enumerate(search_calls()):
                if only is not None and label not in only:
                    continue
                step("search", label, lib.dbgsom_bmu_filtered, x, da.F32, N, d, d, self.xx.data_ptr(), self.pptr,
                     self.live["W"].data_ptr(), M, self.ww.data_ptr(), self.live["prev"].data_ptr() if hinted else None,
                     self.live["order"].data_ptr() if hinted else None, flags, 0, 0,
                     self.idx[i].data_ptr() + wc.PAD * 8, self.dist[i].data_ptr() + wc.PAD * 8, self.ws, self.n)
            step("counts_async", "", lib.dbgsom_bmu_filtered_counts_async, self.ws, N, d, M, self.counts_async.data_ptr(), self.nb)
            self.clones = [(a.clone(), b.clone()) for a, b in zip(self.idx, self.dist)]
        return self

    def read(self, S=None, cycles=0):
        """the blocking readers of the last call's workspace, each behind a sleep of its own"""
        import torch

        lib, inp = self.nat.load(), self.inp
        N, d, M = inp.N, inp.d, inp.M
        stream = self._stream(S)
        s = ctypes.c_void_p(stream.cuda_stream)
        for name in READERS:
            out = self.host_out[name]
            args = (self.ws, N, d, M, out.ctypes.data) + ((self.nb,) if name == "counts" else ())
            with torch.cuda.stream(stream):
                t0 = time.perf_counter()
                if cycles:
                    torch.cuda._sleep(cycles)
                ev = torch.cuda.Event()
                ev.record(stream)
                t1 = time.perf_counter()
                rc = getattr(lib, SEQUENCE_STEPS[name])(*args, s)
                t2 = time.perf_counter()
                self.steps.append((name, "", rc, ev.query(), (t1 - t0) * 1e3, (t2 - t0) * 1e3))
        return self

    def finish(self):
        """-> {name: host array}; the sentinels around every winner and distance vector are checked"""
        import torch

        try:
            self._stream(self.S).synchronize()
            torch.cuda.synchronize()
        except RuntimeError as e:             # a fault of the device: nothing more is started on it in this session
            import pytest

            pytest.exit(f"the filtered sequence, shape {self.inp.si}: the device faulted ({e})", returncode=3)
        N = self.inp.N
        out = dict(self.host_out)
        out["counts_async"] = self.counts_async.numpy().view(np.uint32).copy()
        off = self.ws - self.ws_t.data_ptr()
        out["tickets_zero"] = not self.ws_t[off:off + 256].cpu().numpy().any()
        for i, (label, _, _) in enumerate(search_calls()):
            for kind, bufs, tail in (("idx", (self.clones[i][0], self.idx[i]), wc.TAIL["int64"]),
                                     ("dist", (self.clones[i][1], self.dist[i]), wc.TAIL["float64"])):
                h, late = (t.cpu().numpy() for t in bufs)
                pad = np.full(wc.PAD, np.array(tail, dtype=h.dtype))
                assert wc.same_bits(h[:wc.PAD], pad) and wc.same_bits(h[wc.PAD + N:], pad), f"{label}: a write outside '{kind}'"
                assert wc.same_bits(h, late), f"{label}: '{kind}' changed behind the clone queued after the calls"
                out[f"{kind}:{label}"] = h[wc.PAD:wc.PAD + N].copy()
        return out


# ---- the entries without a workspace: one case each -------------------------------------------------------------------
class PlainRecord:
    """what run of a case needs of a workspace_cases.Record, for an entry that takes no workspace"""

    def __init__(self, entry, case, size_fn=None):
        self.entry, self.cases, self.size_fn = entry, [case], size_fn     # size_fn: the size function of a borrowed workspace

    def nbytes(self, lib, case):
        return int(getattr(lib, self.size_fn)(*case.size_args)) if self.size_fn else 0


PD_CASE = 3          # prototype_distances.CASES[3]: f32, (N, M, d) = (127, 260, 16) -- the workspace table's smallest


def _plain_bmu():
    from tests import kneighbors as kn
    from tests import prototype_distances as pd

    case, N, M, d = wc.pd_case(PD_CASE)
    k = 2

    def inputs():
        X, W, _ = pd.case_data(case)
        return dict(X=X, W=W, xx=wc.row_norms(X), ww=wc.row_norms(W))

    def check(out, inp):                                            # tests/test_gpu_kneighbors.py: columns 0..1 are dbgsom_bmu's
        X, W, D = pd.case_data(case)
        want = kn.topk_oracle(X, W, k, D)
        assert np.array_equal(out["idx"].reshape(N, k), want)
        assert wc.same_bits(out["dist"].reshape(N, k), np.take_along_axis(D, want, axis=1))

    return wc.Case(f"N{N}-M{M}-d{d}-k{k}", (), inputs, {"idx": (N * k, "int64", -7), "dist": (N * k, "float64", float("nan"))},
                   lambda p, ws, nbytes: [p["X"], da.F32, N, d, d, p["xx"], p["W"], M, p["ww"], k, 0, p["idx"], p["dist"]], check,
                   "the register-staged search, two row blocks and three prototype blocks")


def _plain_distances():
    from tests import prototype_distances as pd

    case, N, M, d = wc.pd_case(PD_CASE)

    def inputs():
        X, W, _ = pd.case_data(case)
        return dict(X=X, W=W, xx=wc.row_norms(X), ww=wc.row_norms(W))

    def check(out, inp):                                            # tests/test_gpu_prototype_distances.py: bit for bit
        assert wc.same_bits(out["D"].reshape(N, M), pd.case_data(case)[2])

    return wc.Case(f"N{N}-M{M}-d{d}", (), inputs, {"D": (N * M, "float64", pd.SENTINEL)},
                   lambda p, ws, nbytes: [p["X"], da.F32, N, d, d, p["xx"], p["W"], M, p["ww"], p["D"], M], check,
                   "the store kernel over two row blocks")


def _plain_topk_rows():
    from tests import kneighbors as kn

    case = (300, 63, 4, 3)
    assert case in kn.TOPK_CASES
    N, M, k, _ = case

    def check(out, inp):                                            # tests/test_gpu_kneighbors.py: bit for bit
        want_dist, want_idx = kn.topk_lexsort(inp["R"], k)
        assert np.array_equal(out["idx"].reshape(N, k), want_idx) and wc.same_bits(out["dist"].reshape(N, k), want_dist)

    return wc.Case(f"N{N}-M{M}-k{k}", (), lambda: dict(R=kn.topk_matrix(case)),
                   {"idx": (N * k, "int64", kn.IDX_SENTINEL), "dist": (N * k, "float64", -77.0)},
                   lambda p, ws, nbytes: [p["R"], N, M, M, k, p["idx"], p["dist"]], check, "K = 4 selection, 300 rows")


def _plain_cosine(entry):
    from tests import cosine as cs
    from tests import prototype_distances as pd

    case, N, M, d = wc.pd_case(PD_CASE)
    k = 2

    def inputs():
        X, W, _ = cs.case_data(case)
        return dict(X=X, W=W, u=cs.inv_norms(cs.sqnorm_chain(X)), v=cs.inv_norms(cs.sqnorm_chain(W)))

    if entry == "dbgsom_distances_cosine":
        def check(out, inp):                                        # tests/test_gpu_cosine.py: bit for bit
            assert wc.same_bits(out["D"].reshape(N, M), cs.case_data(case)[2])

        return wc.Case(f"N{N}-M{M}-d{d}", (), inputs, {"D": (N * M, "float64", pd.SENTINEL)},
                       lambda p, ws, nbytes: [p["X"], da.F32, N, d, d, p["u"], p["W"], M, p["v"], p["D"], M], check,
                       "the cosine store kernel")

    def check(out, inp):                                            # tests/test_gpu_cosine.py: bit for bit
        want_dist, want_idx = cs.select(cs.case_data(case)[2], k)
        assert np.array_equal(out["idx"].reshape(N, k), want_idx) and wc.same_bits(out["dist"].reshape(N, k), want_dist)

    return wc.Case(f"N{N}-M{M}-d{d}-k{k}", (), inputs, {"idx": (N * k, "int64", -77), "dist": (N * k, "float64", pd.SENTINEL)},
                   lambda p, ws, nbytes: [p["X"], da.F32, N, d, d, p["u"], p["W"], M, p["v"], k, p["idx"], p["dist"]], check,
                   "the cosine search kernel")


def _plain_inv_norms():
    from tests import cosine as cs
    from tests import prototype_distances as pd

    n = 1000

    def inputs():
        return dict(sq=np.random.default_rng(n).uniform(0.5, 300.0, n))

    def check(out, inp):                                            # tests/test_gpu_cosine.py: sqrt, then the division
        assert np.array_equal(out["out"], cs.inv_norms(inp["sq"]))

    return wc.Case(f"n{n}", (), inputs, {"out": (n, "float64", pd.SENTINEL)},
                   lambda p, ws, nbytes: [p["sq"], n, p["out"]], check, "four workgroups")


def _plain_column_sums():
    N, d = 513, 37
    assert (N, d, 40) in da.COLSUM_SHAPES

    def inputs():
        X = np.random.default_rng(N + d).normal(size=(N, d)) * 2.0 + 0.5
        return dict(X=X, mean=da.column_sums_loop(X) / np.float64(N))

    def check(out, inp):                                            # tests/test_gpu_device_abi.py: NumPy's axis-0 order, bit for bit
        assert np.array_equal(out["out"], da.column_sums_loop(inp["X"], inp["mean"]))

    return wc.Case(f"N{N}-d{d}-f64", (), inputs, {"out": (d, "float64", float("nan"))},
                   lambda p, ws, nbytes: [p["X"], da.F64, N, d, d, p["mean"], p["out"]], check, "squared deviations, float64 rows")


def _plain_range_count_cols():
    from tests import density as dn
    from tests import prototype_distances as pd

    case, N, M, d = wc.pd_case(PD_CASE)
    n_radii = 5

    def inputs():
        D = pd.case_data(case)[2]
        R = np.ascontiguousarray(D * D)
        return dict(R=R, thr=np.quantile(R, [0.05, 0.2, 0.5, 0.5, 0.9]))

    def check(out, inp):                                            # tests/test_gpu_density.py: integer for integer
        want = np.stack([np.count_nonzero(inp["R"] <= t, axis=0) for t in inp["thr"]], axis=1)
        assert np.array_equal(out["counts"].reshape(M, n_radii), want)

    return wc.Case(f"N{N}-M{M}-n{n_radii}", (), inputs, {"counts": (M * n_radii, "int64", 0)},   # (the fold ADDS to its state)
                   lambda p, ws, nbytes: [p["R"], N, M, M, p["thr"], n_radii, p["counts"]], check,
                   "RB = 8 radii, five column blocks; the counts are added to a state of zeros")


# ---- more entries without a workspace of their own ----------------------------------------------------------------
def _plain_edge_lengths():
    from tests import combined_error as ce

    M, d = 70, 17

    def inputs():                                                   # the shapes of tests/test_gpu_combined_error.py
        rng = np.random.default_rng(d)
        W = rng.normal(size=(M, d)) * 10.0 ** rng.integers(-3, 4, size=(M, 1))
        W[9] = W[8]
        edges = np.concatenate([rng.integers(0, M, size=(513, 2)), [[8, 9], [5, 5], [0, M - 1], [M - 1, 0]]]).astype(np.int32)
        return dict(W=W, edges=edges)

    E = 517

    def check(out, inp):                                            # tests/test_gpu_combined_error.py: bit for bit
        assert wc.same_bits(out["len"], ce.edge_lengths(inp["W"], inp["edges"]))

    return wc.Case(f"M{M}-d{d}-E{E}", (), inputs, {"len": (E, "float64", ce.SENTINEL)},
                   lambda p, ws, nbytes: [p["W"], M, d, d, p["edges"], E, p["len"]], check, "three workgroups of edges")


def _plain_combined_error_rows():
    from tests import combined_error as ce

    N, M, ldd = 257, 37, 2

    def inputs():                                                   # the shapes of tests/test_gpu_combined_error.py
        rng = np.random.default_rng(N + ldd)
        G = rng.random((M, M)) * 10.0 ** rng.integers(-3, 4, size=(M, M))
        np.fill_diagonal(G, 0.0)
        idx2 = rng.integers(0, M, size=(N, 2)).astype(np.int64)
        idx2[7] = (-1, 3)
        return dict(idx2=idx2, dist=rng.random((N, ldd)) * 3.0, G=G)

    def check(out, inp):                                            # tests/test_gpu_combined_error.py: bit for bit
        assert wc.same_bits(out["e"], ce.combined_error_rows(inp["idx2"], inp["dist"][:, 0], inp["G"]))

    return wc.Case(f"N{N}-M{M}-ldd{ldd}", (), inputs, {"e": (N, "float64", ce.SENTINEL)},
                   lambda p, ws, nbytes: [p["idx2"], p["dist"], ldd, N, p["G"], M, M, p["e"]], check, "two workgroups of rows")


def _plain_energy_rows():
    from tests import distortion as ds
    from tests import prototype_distances as pd

    case, N, M, d = wc.pd_case(PD_CASE)

    def inputs():
        D = pd.case_data(case)[2]
        return dict(R=np.ascontiguousarray(D * D), H=np.ascontiguousarray(ds.gaussian_factors(M), dtype=np.float64))

    def check(out, inp):                                            # tests/test_gpu_distortion.py: bit for bit
        want_b, want_e = ds.energy_rows(inp["R"], inp["H"])
        assert np.array_equal(out["bmu"], want_b) and wc.same_bits(out["e"], np.asarray(want_e, dtype=np.float64))

    return wc.Case(f"N{N}-M{M}", (), inputs, {"bmu": (N, "int64", ds.BMU_SENTINEL), "e": (N, "float64", ds.SENTINEL)},
                   lambda p, ws, nbytes: [p["R"], N, M, M, p["H"], M, p["bmu"], p["e"]], check, "one wavefront per row")


def _plain_class_histogram():
    from tests import topofn_device as td

    N, M, C = 900, 5, 7
    assert (N, M, C) in td.CLASS_SHAPES

    def inputs():
        winners, y, _ = td.class_inputs(N, M, C)
        return dict(winners=winners, y=y)

    def check(out, inp):                                            # tests/test_gpu_topofn_device.py: exact
        ok = (inp["y"] >= 0) & (inp["y"] < C)
        want = np.bincount(inp["winners"][ok] * C + inp["y"][ok], minlength=M * C)
        assert np.array_equal(out["hist"], want)

    return wc.Case(f"N{N}-M{M}-C{C}", (), inputs, {"hist": (M * C, "int64", -7)},
                   lambda p, ws, nbytes: [p["winners"], p["y"], N, M, C, p["hist"]], check,
                   "the call clears the histogram, then integer atomics from four workgroups")


def _plain_topographic_weight():
    from tests import topofn_device as td

    n = 300000
    assert n in td.TOPO_N

    def inputs():
        idx2, w, xy, M = td.topo_inputs(n, "int")
        return dict(idx2=np.ascontiguousarray(idx2, dtype=np.int64), w=w, xy=np.ascontiguousarray(xy, dtype=np.int32))

    def check(out, inp):                                            # tests/test_gpu_topofn_device.py: integer weights, exact
        idx2, w, xy, M = td.topo_inputs(n, "int")
        assert out["out"][0] == w[td.topo_counted(idx2, xy, M)].sum()

    M = td.topo_inputs(1, "int")[3]
    return wc.Case(f"n{n}", (), inputs, {"out": (1, "float64", float("nan"))},
                   lambda p, ws, nbytes: [p["idx2"], p["w"], n, p["xy"], M, p["out"], ws, nbytes], check,
                   "1024 partials in the workspace of dbgsom_sum_workspace_bytes, a second row per thread")


def _plain_weighted_sum():
    n = 70001
    assert n in da.SUM_N

    def inputs():
        rng = np.random.default_rng(n)
        return dict(v=rng.normal(size=n) * 3.0, w=rng.uniform(0.0, 3.0, n))

    def check(out, inp):                                            # tests/test_gpu_device_abi.py
        from fractions import Fraction

        exact, T = da.exact_sum(inp["v"], inp["w"])
        assert abs(Fraction(float(out["out"][0])) - exact) <= n * Fraction(da.U) * T

    return wc.Case(f"n{n}", (), inputs, {"out": (1, "float64", float("nan"))},
                   lambda p, ws, nbytes: [p["v"], p["w"], n, p["out"], ws, nbytes], check, "1024 partials in the workspace")


def _plain_distances_manhattan():
    from tests import manhattan as mh

    dtype, N, d, M = "f64", 17, 33, 257

    def inputs():
        X, W = mh.raw_case(dtype, N, d, M)
        return dict(X=X, W=W)

    def check(out, inp):                                            # tests/test_gpu_manhattan.py: bit for bit
        assert wc.same_bits(out["D"].reshape(N, M), np.asarray(mh.raw_reference(dtype, N, d, M), dtype=np.float64))

    return wc.Case(f"{dtype}-N{N}-d{d}-M{M}", (da.CODE[dtype], N, d, M), inputs, {"D": (N * M, "float64", -77.0)},
                   lambda p, ws, nbytes: [p["X"], da.CODE[dtype], N, d, d, p["W"], M, d, p["D"], M, ws, nbytes], check,
                   "Wt in the workspace, two prototype blocks")


def _plain_distances_masked():
    from tests import test_missing_cpu as tm

    N, d, M, dtype_name = 257, 17, 5, "float64"

    def inputs():
        X, W, _ = tm.case(N, d, M, 0.3, dtype_name)
        return dict(X=X, W=W)

    def check(out, inp):                                            # tests/test_gpu_prototype_distances.py
        np.testing.assert_allclose(out["D"].reshape(N, M), tm.case(N, d, M, 0.3, dtype_name)[2], rtol=tm.RTOL, atol=0.0)

    return wc.Case(f"N{N}-d{d}-M{M}-{dtype_name}", (da.F64, N, d, M), inputs, {"D": (N * M, "float64", float("nan"))},
                   lambda p, ws, nbytes: [p["X"], da.F64, N, d, d, p["W"], M, d, p["D"], M, ws, nbytes], check,
                   "Wt and n_obs in the workspace, rows with missing entries")


def _plain_topographic_count():
    from tests import topofn_device as td

    n = 300000

    def inputs():
        idx2, _, xy, _ = td.topo_inputs(n, "int")
        return dict(idx2=np.ascontiguousarray(idx2, dtype=np.int64), xy=np.ascontiguousarray(xy, dtype=np.int32))

    def check(out, inp):                                            # tests/test_gpu_topofn_device.py: exact
        idx2, _, xy, M = td.topo_inputs(n, "int")
        assert int(out["count"][0]) == int(td.topo_counted(idx2, xy, M).sum())

    M = td.topo_inputs(1, "int")[3]
    return wc.Case(f"n{n}", (), inputs, {"count": (1, "int64", -7)},
                   lambda p, ws, nbytes: [p["idx2"], n, p["xy"], M, p["count"]], check,
                   "the call clears the counter, then integer atomics; every input shapes memory access (no decoy)")


def _plain_elementwise(entry):
    n, sigma, gamma = 1000, 1.3, 0.37

    def inputs():                                                   # the inputs of tests/test_gpu_device_abi.py
        dist = 3.0 * np.random.default_rng(n).random(n)
        dist[0] = 0.0
        return dict(dist=dist)

    if entry == "dbgsom_density_terms":
        def check(out, inp):                                        # tests/test_gpu_device_abi.py
            want = np.exp(-(inp["dist"] ** 2) / (2 * sigma ** 2)) / (sigma * np.sqrt(2 * np.pi))
            np.testing.assert_allclose(out["out"], want, rtol=1e-13)
        scalar = sigma
    else:
        def check(out, inp):                                        # tests/test_gpu_device_abi.py
            from oracle import som_oracle as o

            np.testing.assert_allclose(out["out"], o.exp_similarity_gamma(inp["dist"], gamma), rtol=1e-13, atol=1e-16)
        scalar = gamma
    return wc.Case(f"n{n}", (), inputs, {"out": (n, "float64", float("nan"))},
                   lambda p, ws, nbytes: [p["dist"], n, scalar, p["out"]], check, "four workgroups")


def _plain_class_histogram_weighted():
    from tests import topofn_device as td

    N, M, C = 900, 5, 7
    assert (N, M, C) in td.CLASS_SHAPES

    def inputs():
        winners, y, w = td.class_inputs(N, M, C, integer_weights=True)
        order, seg = td.bucket(winners, M)
        return dict(order=np.ascontiguousarray(order, dtype=np.int32), seg_start=np.ascontiguousarray(seg, dtype=np.uint32), y=y, w=w)

    def check(out, inp):                                            # tests/test_gpu_topofn_device.py: integer weights, exact
        winners, y, w = td.class_inputs(N, M, C, integer_weights=True)
        ok = (y >= 0) & (y < C)
        want = np.zeros((M, C))
        np.add.at(want, (winners[ok], y[ok]), w[ok])
        assert np.array_equal(out["hist"].reshape(M, C), want)

    return wc.Case(f"N{N}-M{M}-C{C}", (), inputs, {"hist": (M * C, "float64", float("nan"))},
                   lambda p, ws, nbytes: [p["order"], p["seg_start"], p["y"], p["w"], N, M, C, p["hist"]], check,
                   "one workgroup per neuron, lists of several tiles")


# ---- the CSR kernels, the fill, the slab drivers over the distortion and the mixture --------------------------------
def _plain_csr_row_sqnorms():
    from tests import csr_device as cd

    N = 257
    assert N in cd.NORM_N

    @functools.lru_cache(maxsize=None)
    def matrix():
        rng = np.random.default_rng(N)
        return cd.rows_csr(cd.norm_lengths(N, rng), cd.NORM_D, "f64", rng, stored_zeros=5)

    def inputs():
        indptr, _, data = cd.arrays(matrix())
        return dict(indptr=indptr, data=data)

    def check(out, inp):                                            # tests/test_gpu_csr_device.py: the chain, bit for bit
        from oracle import som_oracle as o

        assert np.array_equal(out["out"], o.row_sqnorms_chain(matrix().toarray()))

    return wc.Case(f"N{N}-d{cd.NORM_D}-f64", (), inputs, {"out": (N, "float64", float("nan"))},
                   lambda p, ws, nbytes: [p["indptr"], p["data"], da.F64, N, p["out"]], check,
                   "two workgroups, the long last row behind the first")


def _plain_csr_transpose_weights():
    from tests import csr_device as cd

    M, d = 257, 40
    ldwt = cd.wt_ld(M)

    def check(out, inp):                                            # tests/test_gpu_csr_device.py
        body = out["Wt"].reshape(d, ldwt)
        assert np.array_equal(body[:, :M], inp["W"].T) and (body[:, M:] == 0).all()

    return wc.Case(f"M{M}-d{d}", (), lambda: dict(W=np.random.default_rng(M + d).normal(size=(M, d))),
                   {"Wt": (d * ldwt, "float64", float("nan"))},
                   lambda p, ws, nbytes: [p["W"], M, d, d, p["Wt"], ldwt], check, "several tiles, zeros behind column M")


def _plain_bmu_csr():
    from tests import csr_device as cd

    row = ("f64", 129, 37, 513, 1, 0)
    assert row in cd.BMU_CSR_CASES
    dtype, N, d, M, k, round_f32 = row
    ldwt = cd.wt_ld(M)

    @functools.lru_cache(maxsize=None)
    def data():
        return cd.search_case(*row)

    def inputs():
        from oracle import som_oracle as o

        X, W = data()
        indptr, indices, vals = cd.arrays(X)
        Wt = np.zeros((d, ldwt))
        Wt[:, :M] = W.T
        return dict(indptr=indptr, indices=indices, data=vals, xx=o.row_sqnorms_chain(X.toarray()), Wt=Wt,
                    ww=o.row_sqnorms_chain(W))

    def check(out, inp):                                            # tests/test_gpu_csr_device.py: the chain, bit for bit
        from oracle import som_oracle as o

        X, W = data()
        rd, ri = o.bmu_chain(X.toarray(), W, k)
        assert np.array_equal(out["idx"], ri.reshape(-1)) and wc.same_bits(out["dist"], np.ascontiguousarray(rd).reshape(-1))

    return wc.Case(f"{dtype}-N{N}-d{d}-M{M}-k{k}", (), inputs, {"idx": (N * k, "int64", -7), "dist": (N * k, "float64", float("nan"))},
                   lambda p, ws, nbytes: [p["indptr"], p["indices"], p["data"], da.F64, N, p["xx"], p["Wt"], ldwt, M, p["ww"], k,
                                          round_f32, p["idx"], p["dist"]], check, "two row blocks, several prototype blocks")


def _plain_csr_densify():
    from tests import csr_device as cd

    N, d, ld = 9, 200, 203
    assert (N, d, ld) in cd.DENSIFY_SHAPES

    @functools.lru_cache(maxsize=None)
    def matrix():
        rng = np.random.default_rng(N + d)
        return cd.rows_csr(cd.densify_lengths(N, d, rng), d, "f64", rng, stored_zeros=2)

    def inputs():
        indptr, indices, data = cd.arrays(matrix())
        return dict(indptr=indptr, indices=indices, data=data)

    def check(out, inp):                                            # tests/test_gpu_csr_device.py
        body = out["rows"].reshape(N, ld)
        assert np.array_equal(body[:, :d], matrix().toarray()) and (body[:, d:] == 0).all()

    return wc.Case(f"N{N}-d{d}-ld{ld}-f64", (), inputs, {"rows": (N * ld, "float64", float("nan"))},
                   lambda p, ws, nbytes: [p["indptr"], p["indices"], p["data"], da.F64, N, d, ld, p["rows"]], check,
                   "the call clears the rows, then scatters the stored entries")


def _plain_fill_missing():
    from tests import test_missing_cpu as tm

    N, d, M, dtype_name = 257, 17, 5, "float64"

    def inputs():
        X, W, D = tm.case(N, d, M, 0.3, dtype_name)
        return dict(X=X, W=W, idx=np.ascontiguousarray(tm.winners_of(D, 1)[1].reshape(N, 1), dtype=np.int64))

    def check(out, inp):                                            # tests/test_gpu_missing.py: the holes get the winner's entries
        assert wc.same_bits(out["X"].reshape(N, d), tm.fill_numpy(inp["X"], inp["W"], inp["idx"][:, 0]))

    case = wc.Case(f"N{N}-d{d}-M{M}-{dtype_name}", (), inputs, {},
                   lambda p, ws, nbytes: [p["X"], da.F64, N, d, d, p["W"], M, d, p["idx"], 1], check, "rows filled in place")
    case.inout = ("X",)                                             # read back from its live buffer behind the entry
    return case


def _plain_neighborhood_energy():
    from tests import distortion as ds
    from tests import prototype_distances as pd

    case, N, M, d = wc.pd_case(PD_CASE)

    def inputs():
        X, W, _ = pd.case_data(case)
        return dict(X=X, W=W, xx=wc.row_norms(X), ww=wc.row_norms(W), H=np.ascontiguousarray(ds.case_reference(case)[1], dtype=np.float64))

    def check(out, inp):                                            # tests/test_gpu_distortion.py: bit for bit
        _, _, want_b, want_e = ds.case_reference(case)
        assert np.array_equal(out["bmu"], want_b) and wc.same_bits(out["e"], np.asarray(want_e, dtype=np.float64))

    return wc.Case(f"N{N}-M{M}-d{d}", (N, M, 0), inputs, {"bmu": (N, "int64", ds.BMU_SENTINEL), "e": (N, "float64", ds.SENTINEL)},
                   lambda p, ws, nbytes: [p["X"], da.F32, N, d, d, p["xx"], p["W"], M, p["ww"], p["H"], M, 0, p["bmu"], p["e"], ws,
                                          nbytes], check, "one slab in the workspace, then the energy kernel")


def _check_mixture(R, a, c, Y, out, N, nv):
    from tests import mixture as mx

    unit, lse, q = out["unit"], out["lse"], out["q"].reshape(N, nv)
    assert np.array_equal(unit, mx.mixture_rows(R, a, c, Y)[0])     # tests/test_gpu_mixture.py: _check_general
    rows = mx.defined(R, a, c)
    assert np.isnan(lse[~rows]).all() and np.isnan(q[~rows]).all() and np.isfinite(lse[rows]).all() and np.isfinite(q[rows]).all()
    if da.have_longdouble():
        mx.check_outputs(R, a, c, Y, unit, lse, q, mx.E_DEVICE)


def _plain_mixture_rows():
    from tests import mixture as mx

    row = (9, 65, 4, False)
    assert row in mx.ROWS_CASES
    N, M, nv, _ = row

    def inputs():
        R, a, c, Y = mx.rows_problem(row)
        return dict(R=np.ascontiguousarray(R), a=np.asarray(a, dtype=np.float64), Y=np.ascontiguousarray(Y, dtype=np.float64))

    c = float(mx.rows_problem(row)[2])

    def check(out, inp):
        _check_mixture(inp["R"], inp["a"], c, inp["Y"], out, N, nv)

    return wc.Case(f"N{N}-M{M}-V{nv}", (), inputs,
                   {"unit": (N, "int64", -7), "lse": (N, "float64", -1234.5), "q": (N * nv, "float64", -1234.5)},
                   lambda p, ws, nbytes: [p["R"], N, M, M, p["a"], c, p["Y"], nv, nv, p["unit"], p["lse"], p["q"], nv], check,
                   "a wavefront per row, three workgroups, two values per lane")


def _plain_mixture():
    from tests import mixture as mx
    from tests import prototype_distances as pd

    case, N, M, d = wc.pd_case(PD_CASE)
    nv = 3

    def inputs():
        X, W, _ = pd.case_data(case)
        R, a, c, Y = mx.case_reference(case, nv)[:4]
        return dict(X=X, W=W, xx=wc.row_norms(X), ww=wc.row_norms(W), a=np.asarray(a, dtype=np.float64),
                    Y=np.ascontiguousarray(Y, dtype=np.float64))

    c = float(mx.case_reference(case, nv)[2])

    def check(out, inp):
        R = mx.case_reference(case, nv)[0]
        _check_mixture(R, inp["a"], c, inp["Y"], out, N, nv)

    return wc.Case(f"N{N}-M{M}-d{d}-V{nv}", (N, M, 0), inputs,
                   {"unit": (N, "int64", -7), "lse": (N, "float64", -1234.5), "q": (N * nv, "float64", -1234.5)},
                   lambda p, ws, nbytes: [p["X"], da.F32, N, d, d, p["xx"], p["W"], M, p["ww"], p["a"], c, p["Y"], nv, nv, 0, p["unit"],
                                          p["lse"], p["q"], nv, ws, nbytes], check, "one slab in the workspace, then the mixture kernel")


_PLAIN = None


def plain_records():
    """-> {entry: PlainRecord}"""
    global _PLAIN
    if _PLAIN is None:
        made = {
            "dbgsom_bmu": _plain_bmu(), "dbgsom_distances": _plain_distances(), "dbgsom_topk_rows": _plain_topk_rows(),
            "dbgsom_distances_cosine": _plain_cosine("dbgsom_distances_cosine"), "dbgsom_bmu_cosine": _plain_cosine("dbgsom_bmu_cosine"),
            "dbgsom_inv_norms": _plain_inv_norms(), "dbgsom_column_sums": _plain_column_sums(),
            "dbgsom_range_count_cols": _plain_range_count_cols(), "dbgsom_edge_lengths": _plain_edge_lengths(),
            "dbgsom_combined_error_rows": _plain_combined_error_rows(), "dbgsom_energy_rows": _plain_energy_rows(),
            "dbgsom_class_histogram": _plain_class_histogram(), "dbgsom_topographic_weight": _plain_topographic_weight(),
        }
        made.update({"dbgsom_weighted_sum_f64": _plain_weighted_sum(), "dbgsom_distances_manhattan": _plain_distances_manhattan(),
                     "dbgsom_distances_masked": _plain_distances_masked(), "dbgsom_topographic_count": _plain_topographic_count()})
        made.update({"dbgsom_exp_similarity": _plain_elementwise("dbgsom_exp_similarity"),
                     "dbgsom_density_terms": _plain_elementwise("dbgsom_density_terms"),
                     "dbgsom_class_histogram_weighted": _plain_class_histogram_weighted()})
        made.update({"dbgsom_csr_row_sqnorms": _plain_csr_row_sqnorms(), "dbgsom_csr_transpose_weights": _plain_csr_transpose_weights(),
                     "dbgsom_bmu_csr": _plain_bmu_csr(), "dbgsom_csr_densify": _plain_csr_densify(),
                     "dbgsom_fill_missing": _plain_fill_missing(), "dbgsom_neighborhood_energy": _plain_neighborhood_energy(),
                     "dbgsom_mixture_rows": _plain_mixture_rows(), "dbgsom_mixture": _plain_mixture()})
        sized = {"dbgsom_neighborhood_energy": "dbgsom_kneighbors_workspace_bytes", "dbgsom_mixture": "dbgsom_kneighbors_workspace_bytes",
                 "dbgsom_topographic_weight": "dbgsom_sum_workspace_bytes", "dbgsom_weighted_sum_f64": "dbgsom_sum_workspace_bytes",
                 "dbgsom_distances_manhattan": "dbgsom_bmu_manhattan_workspace_bytes",
                 "dbgsom_distances_masked": "dbgsom_bmu_masked_workspace_bytes"}
        _PLAIN = {entry: PlainRecord(entry, case, sized.get(entry)) for entry, case in made.items()}
    return _PLAIN


def record(name):
    """a size function of workspace_cases.records() or an entry of plain_records() -> the record"""
    return wc.records()[name] if name in wc.records() else plain_records()[name]


def all_keys():
    """(record name, case index) of every case run behind the delay"""
    return cases() + [(entry, 0) for entry in plain_records()]


def key_id(key):
    return wc.case_id(key) if key[0] in wc.records() else key[0][len("dbgsom_"):] + ":" + record(key[0]).cases[0].label


# ---- the anchored forms of the filtered family: a second sequence, on the workspace they share with it ----------------
ANCHORED_SHAPE = 3                   # filter_device.RAW_SHAPES[3]: (1000, 48, 300), 8 workgroups, d a multiple of 16
ANCHORS = 64
ANCHORED_STEPS = {
    "norms": "dbgsom_row_sqnorms", "prepare": "dbgsom_filter_prepare", "runs_build": "dbgsom_anchor_runs_build",
    "anchored": "dbgsom_bmu_filtered_anchored", "anchor_runs": "dbgsom_bmu_filtered_anchor_runs",
    "anchor_seeds": "dbgsom_bmu_filtered_anchor_seeds", "anchor_bounds": "dbgsom_bmu_filtered_anchor_bounds",
    "runs_read": "dbgsom_anchor_runs_read",
}
ANCHORED_READERS = ("anchor_seeds", "anchor_bounds", "runs_read")
BLOCKS.update({
    "dbgsom_bmu_filtered_anchor_seeds": "Synchronises the stream.",
    "dbgsom_bmu_filtered_anchor_bounds": "Synchronises the stream.",
    "dbgsom_anchor_runs_read": "are written. Synchronises.",
})
ANCHORED_FIXED = {"anchor_of": "shapes memory access", "order": "shapes memory access"}


class AnchoredInputs:
    """rows, prototypes padded to whole 64 rows (zeros behind M, as the context keeps them), anchors and buckets of one
    shape, their decoys and the chain reference; device copies made once, read only"""

    def __init__(self, si=ANCHORED_SHAPE, A=ANCHORS):
        from oracle import som_oracle as o
        from tests import anchor_mark as am
        from tests import filter_device as fd

        self.si, self.A = si, A
        self.N, self.d, self.M = fd.RAW_SHAPES[si]
        assert self.d % 16 == 0
        X, W = fd.raw_data(si, "f32")
        self.ref_dist, self.ref_idx = o.bmu_chain(X, W, 1)
        self.Mg = (self.M + 63) // 64 * 64
        Wg = np.zeros((self.Mg, self.d))
        Wg[:self.M] = W
        anchors, aof, order = am.buckets(np.ascontiguousarray(X), A)
        assert anchors.shape == (A, self.d)
        self.host = dict(X=np.ascontiguousarray(X), W=Wg, anchors=np.ascontiguousarray(anchors, dtype=np.float64),
                         anchor_of=np.ascontiguousarray(aof, dtype=np.int32), order=np.ascontiguousarray(order, dtype=np.int32))
        self.decoys = {k: (v.copy() if k in ANCHORED_FIXED else decoy(k, v)) for k, v in self.host.items()}
        self.decoys["W"][self.M:] = 0.0                             # (the padding rows stay zeros)
        self._dev = None

    def dev(self):
        if self._dev is None:
            self._dev = ({k: da.dev(v) for k, v in self.host.items()}, {k: da.dev(v) for k, v in self.decoys.items()})
        return self._dev


class AnchoredRun:
    """one run: prepare (null stream) -> the caller synchronises -> launch_searches (norms, planes, the run table, the
    anchored search, the search over the run table: enqueue-only) -> read (the blocking readers, each behind a delay of
    its own) -> finish"""

    def __init__(self, nat, inp):
        import torch

        self.nat, self.inp = nat, inp
        N, d, M, Mg, A = inp.N, inp.d, inp.M, inp.Mg, inp.A
        lib = nat.load()
        self.live = {k: t.clone() for k, t in inp.dev()[1].items()}
        self.xx = torch.full((N,), -1.0, dtype=torch.float64, device="cuda")
        self.ww = torch.full((Mg,), -1.0, dtype=torch.float64, device="cuda")
        self.pbytes = int(lib.dbgsom_filter_planes_bytes(N, d))
        self.planes = torch.zeros(self.pbytes + 512, dtype=torch.uint8, device="cuda")
        self.pptr = (self.planes.data_ptr() + 255) // 256 * 256
        self.rbytes = int(lib.dbgsom_anchor_runs_bytes(N, A))
        self.runs = torch.zeros(self.rbytes + 512, dtype=torch.uint8, device="cuda")
        self.rptr = (self.runs.data_ptr() + 255) // 256 * 256
        self.n = int(lib.dbgsom_bmu_filtered_workspace_bytes(N, d, M))
        self.ws_t = torch.full((self.n + 256,), 0xFF, dtype=torch.uint8, device="cuda")   # zero-filled once: on the stream
        self.ws = (self.ws_t.data_ptr() + 255) // 256 * 256
        self.idx = [torch.full((N + 2 * wc.PAD,), wc.TAIL["int64"], dtype=torch.int64, device="cuda") for _ in range(2)]
        self.dist = [torch.full((N + 2 * wc.PAD,), wc.TAIL["float64"], dtype=torch.float64, device="cuda") for _ in range(2)]
        self.nb = (N + 127) // 128
        cap = self.nb + A
        self.host_out = {"aseed": np.full(A, -7, dtype=np.int32), "low": np.full((A, M), np.nan, dtype=np.float32),
                         "up": np.full(A, np.nan), "handed": np.zeros(2, dtype=np.uint64),
                         "run_start": np.full(self.nb + 1, -7, dtype=np.int32), "run_anchor": np.full(cap, -7, dtype=np.int32),
                         "run_R": np.full(cap, np.nan), "run_xx": np.full(cap, np.nan)}
        self.steps, self.events = [], {}

    def _stream(self, S):
        import torch

        return torch.cuda.current_stream() if S is None else S

    def launch_searches(self, S=None, cycles=0, keep_decoy=()):
        import torch

        from tests import filter_device as fd

        lib, inp = self.nat.load(), self.inp
        N, d, M, A = inp.N, inp.d, inp.M, inp.A
        true = inp.dev()[0]
        self.S = S
        stream = self._stream(S)
        s = ctypes.c_void_p(stream.cuda_stream)
        with torch.cuda.stream(stream):
            t0 = time.perf_counter()
            if cycles:
                torch.cuda._sleep(cycles)
            for k, t in self.live.items():
                if k not in keep_decoy:
                    t.copy_(true[k])
            self.ws_t.zero_()
            self.planes.fill_(0x7f)
            self.runs.fill_(0x7f)
            self.xx.fill_(float("nan"))
            self.ww.zero_()
            for i in range(2):
                self.idx[i][wc.PAD:wc.PAD + N] = -7
                self.dist[i][wc.PAD:wc.PAD + N] = float("nan")

            def step(name, label, fn, *args):
                ev = torch.cuda.Event()
                ev.record(stream)
                t1 = time.perf_counter()
                rc = fn(*args, s)
                t2 = time.perf_counter()
                self.steps.append((name, label, rc, ev.query(), (t1 - t0) * 1e3, (t2 - t0) * 1e3))

            L = self.live
            x, w, an, of, order = (L[k].data_ptr() for k in ("X", "W", "anchors", "anchor_of", "order"))
            step("norms", "X", lib.dbgsom_row_sqnorms, x, da.F32, N, d, d, self.xx.data_ptr())
            step("norms", "W", lib.dbgsom_row_sqnorms, w, da.F64, M, d, d, self.ww.data_ptr())
            step("prepare", "X", lib.dbgsom_filter_prepare, x, da.F32, N, d, d, self.pptr, self.pbytes)
            step("runs_build", "", lib.dbgsom_anchor_runs_build, x, da.F32, N, d, d, self.xx.data_ptr(), an, A, of, order,
                 self.rptr, self.rbytes)
            out = lambda i: (self.idx[i].data_ptr() + wc.PAD * 8, self.dist[i].data_ptr() + wc.PAD * 8)   # noqa: E731
            step("anchored", "", lib.dbgsom_bmu_filtered_anchored, x, da.F32, N, d, d, self.xx.data_ptr(), self.pptr, w, M,
                 self.ww.data_ptr(), an, A, of, order, fd.PRUNE, 0, 0, *out(0), self.ws, self.n)
            step("anchor_runs", "", lib.dbgsom_bmu_filtered_anchor_runs, x, da.F32, N, d, d, self.xx.data_ptr(), self.pptr, w, M,
                 self.ww.data_ptr(), an, A, of, order, self.rptr, fd.PRUNE, 0, 0, *out(1), self.ws, self.n)
            self.clones = [(a.clone(), b.clone()) for a, b in zip(self.idx, self.dist)]
        return self

    def read(self, S=None, cycles=0):
        import torch

        lib, inp, h = self.nat.load(), self.inp, self.host_out
        N, d, M, A = inp.N, inp.d, inp.M, inp.A
        stream = self._stream(S)
        s = ctypes.c_void_p(stream.cuda_stream)
        calls = {
            "anchor_seeds": (self.ws, N, d, M, A, h["aseed"].ctypes.data, None),
            "anchor_bounds": (self.ws, N, d, M, A, h["low"].ctypes.data, h["up"].ctypes.data, h["handed"].ctypes.data),
            "runs_read": (self.rptr, N, A, h["run_start"].ctypes.data, h["run_anchor"].ctypes.data, h["run_R"].ctypes.data,
                          h["run_xx"].ctypes.data),
        }
        for name in ANCHORED_READERS:
            with torch.cuda.stream(stream):
                t0 = time.perf_counter()
                if cycles:
                    torch.cuda._sleep(cycles)
                ev = torch.cuda.Event()
                ev.record(stream)
                t1 = time.perf_counter()
                rc = getattr(lib, ANCHORED_STEPS[name])(*calls[name], s)
                t2 = time.perf_counter()
                self.steps.append((name, "", rc, ev.query(), (t1 - t0) * 1e3, (t2 - t0) * 1e3))
        return self

    def finish(self):
        """-> {name: host array}; sentinels around the winners and distances, and the bytes behind the run table, checked"""
        import torch

        try:
            self._stream(self.S).synchronize()
            torch.cuda.synchronize()
        except RuntimeError as e:             # a fault of the device: nothing more is started on it in this session
            import pytest

            pytest.exit(f"the anchored sequence: the device faulted ({e})", returncode=3)
        N = self.inp.N
        out = dict(self.host_out)
        n = int(out["run_start"][-1])
        assert 0 < n <= self.nb + self.inp.A
        for k in ("run_anchor", "run_R", "run_xx"):                  # (only the first run_start[last] entries are written)
            out[k] = out[k][:n].copy()
        off = self.rptr - self.runs.data_ptr()
        assert (self.runs[off + self.rbytes:].cpu().numpy() == 0x7f).all(), "dbgsom_anchor_runs_build wrote behind its table"
        off = self.ws - self.ws_t.data_ptr()
        out["tickets_zero"] = not self.ws_t[off:off + 256].cpu().numpy().any()
        out["xx"] = self.xx.cpu().numpy()
        for i, label in enumerate(("anchored", "anchor_runs")):
            for kind, bufs, tail in (("idx", (self.clones[i][0], self.idx[i]), wc.TAIL["int64"]),
                                     ("dist", (self.clones[i][1], self.dist[i]), wc.TAIL["float64"])):
                h, late = (t.cpu().numpy() for t in bufs)
                pad = np.full(wc.PAD, np.array(tail, dtype=h.dtype))
                assert wc.same_bits(h[:wc.PAD], pad) and wc.same_bits(h[wc.PAD + N:], pad), f"{label}: a write outside '{kind}'"
                assert wc.same_bits(h, late), f"{label}: '{kind}' changed behind the clone queued after the calls"
                out[f"{kind}:{label}"] = h[wc.PAD:wc.PAD + N].copy()
        return out
