"""MI355X: the stream contract of include/dbgsom_hip.h ("device-level calls only ENQUEUE work on `stream`; the caller
synchronises") on a busy non-blocking stream -- the rig of tests/stream_cases.py, DESIGN.md 6.5.

A. every case of tests/workspace_cases.py that goes through run_case, behind a delay on the stream of a context:
   status 0, pads intact, the outputs of the null-stream run bit for bit, the gate of the entry's own GPU test, and the
   entry waited for its stream exactly where the header says it does.  The null-stream run comes first (warm-up, the
   bits to compare with, the host time the call takes); beside it the sensitivity control: each decoy alone changes
   an output bit, or the table says why it cannot.
B. two streams at once: case 0 of a record on one stream and case 1 on another, each behind its own delay, queued
   in both orders from one host thread: the bits of the solo runs (state hidden behind the ABI -- set-once launch
   attributes, thread-local helpers -- would show here).

Every test depends on the rig's self-test, which FAILS where the null stream and the stream do not run
independently or the delay is not real: a blind rig must not pass."""
import numpy as np
import pytest

from tests import stream_cases as sc
from tests import workspace_cases as wc

pytestmark = pytest.mark.gpu

CASES = sc.all_keys()
RECORDS = list(dict.fromkeys(name for name, _ in sc.cases()))
_NULL = {}          # (size function, case index) -> (outputs of the null-stream run, host ms of the call)


@pytest.fixture(scope="session")
def nat():
    from dbgsom_amd import _native

    _native.load()
    return _native


@pytest.fixture(scope="session")
def rig(nat):
    """the streams, the calibrated delay and the self-test: a sleep and a copy into a live buffer on S; a clone on the
    null stream behind them must still see the decoy, and an event on S behind the sleep must be incomplete"""
    import torch

    r = sc.Rig(nat)
    try:
        S = r.stream(0)
        ms0 = r.calibrate()
        live = torch.full((4096,), 1.0, dtype=torch.float64, device="cuda")      # the decoy
        true = torch.full((4096,), 2.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ev = torch.cuda.Event()
        with torch.cuda.stream(S):
            torch.cuda._sleep(r.cycles())
            live.copy_(true)
            ev.record(S)
        seen = live.clone()                                   # on the null stream
        torch.cuda.default_stream().synchronize()             # the null stream only
        behind = ev.query()
        seen_h = seen.cpu().numpy()
        S.synchronize()
        print(f"stream rig: _sleep({sc.SLEEP_C0}) = {ms0:.3f} ms, {r.cycles_per_ms:.0f} cycles / ms, D = {sc.D_MS} ms")
        assert not behind, "rig self-test: the event behind the sleep was complete once the null stream was: no delay"
        assert (seen_h == 1.0).all(), "rig self-test: the null stream waited for the non-blocking stream (saw the true values)"
        assert (live.cpu().numpy() == 2.0).all()
        yield r
    finally:
        r.close()


def _null_run(nat, key):
    if key not in _NULL:
        rec = sc.record(key[0])
        case = rec.cases[key[1]]
        r = sc.enqueue(nat, rec, case)
        out = sc.finish(r)
        assert r.rc == 0, f"{rec.entry} {case.label} (null stream): status {r.rc}: {nat.load().dbgsom_last_error()}"
        _NULL[key] = (out, (r.t_ret - r.t_call) * 1e3)
    return _NULL[key]


def _same(rec, case, got, want, what):
    for name in want:
        assert wc.same_bits(got[name], want[name]), \
            f"{rec.entry} {case.label}: output '{name}' {what} differs from the null-stream run " \
            f"({int((got[name] != want[name]).sum())} of {got[name].size} elements)"


# ---- A. one entry behind the delay ----------------------------------------------------------------------------------
@pytest.mark.parametrize("key", CASES, ids=[sc.key_id(k) for k in CASES])
def test_entry_behind_a_delay_on_a_non_blocking_stream(nat, rig, key):
    rec = sc.record(key[0])
    case = rec.cases[key[1]]
    null, call_ms = _null_run(nat, key)
    print(f"{rec.entry} {case.label}: the call took {call_ms:.3f} ms to return on the null stream")
    if rec.entry not in sc.BLOCKS:
        assert sc.MARGIN * call_ms <= sc.D_MS, f"{rec.entry} {case.label}: delay too short for a call of {call_ms:.2f} ms"
    # the sensitivity control: every decoy alone is seen
    seen = []
    for name, v in sc.live_inputs(case).items():
        if name in sc.FIXED:
            continue
        r = sc.enqueue(nat, rec, case, keep_decoy=(name,))
        out = sc.finish(r)
        differs = r.rc != 0 or any(not wc.same_bits(out[o], null[o]) for o in null)
        why = sc.unobservable(rec, case, name)
        assert differs != bool(why), f"{rec.entry} {case.label}: the decoy of '{name}' " + \
            ("changes the result, yet the table calls it unobservable" if differs else "changes no output bit")
        seen += [name] if differs else []
    decoyable = [k for k in sc.live_inputs(case) if k not in sc.FIXED]
    assert seen or not decoyable, f"{rec.entry} {case.label}: no input of this case is observable"
    # the run behind the delay
    r = sc.enqueue(nat, rec, case, rig.stream(0), rig.cycles())
    out = sc.finish(r)
    assert r.rc == 0, f"{rec.entry} {case.label}: status {r.rc}: {nat.load().dbgsom_last_error()}"
    sc.check_delay(r)
    _same(rec, case, out, null, "behind the delay")
    case.check(out, case.inputs())


# ---- B. two streams at once -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["AB", "BA"])
@pytest.mark.parametrize("name", RECORDS, ids=[n[len("dbgsom_"):-len("_bytes")].replace("_workspace", "") for n in RECORDS])
def test_two_cases_on_two_streams_at_once(nat, rig, name, order):
    import torch

    rec = wc.records()[name]
    runs = {"A": (rec.cases[0], rig.stream(1), (name, 0)), "B": (rec.cases[1], rig.stream(2), (name, 1))}
    null = {tag: _null_run(nat, key)[0] for tag, (_, _, key) in runs.items()}
    pending = {tag: sc.prepare(nat, rec, runs[tag][0]) for tag in order}
    torch.cuda.synchronize()
    for tag in order:                                         # one host thread: queued one after the other
        sc.launch(pending[tag], runs[tag][1], rig.cycles())
    outs = {tag: sc.finish(pending[tag]) for tag in order}
    for tag in order:
        r, case = pending[tag], runs[tag][0]
        assert r.rc == 0, f"{rec.entry} {case.label} ({order}): status {r.rc}: {nat.load().dbgsom_last_error()}"
        sc.check_delay(r, f" ({tag} of {order})")
        _same(rec, case, outs[tag], null[tag], f"with the other case on a second stream ({tag} of {order})")


# ---- the filtered family as one sequence ------------------------------------------------------------------------------
_SEQ_INPUTS, _SEQ_NULL = {}, {}


def _seq_inputs(si):
    if si not in _SEQ_INPUTS:
        _SEQ_INPUTS[si] = sc.FilteredInputs(si)
    return _SEQ_INPUTS[si]


def _seq_run(nat, si, streams=None, cycles=0, keep_decoy=()):
    import torch

    run = sc.FilteredRun(nat, _seq_inputs(si))
    torch.cuda.synchronize()
    run.launch_searches(streams, cycles, keep_decoy).read(streams, cycles)
    return run, run.finish()


def _seq_steps(run, delayed, what):
    table = sc.ANCHORED_STEPS if isinstance(run, sc.AnchoredRun) else sc.SEQUENCE_STEPS
    for name, label, rc, done, ms_call, ms_ret in run.steps:
        entry = table[name]
        assert rc == 0, f"{entry} {label} ({what}): status {rc}: {run.nat.load().dbgsom_last_error()}"
        if not delayed:
            continue
        blocking = entry in sc.BLOCKS
        host_ms = ms_call if blocking else ms_ret
        assert host_ms < sc.D_MS / 2, f"{entry} {label} ({what}): delay too short ({host_ms:.2f} ms of host work, D = {sc.D_MS} ms)"
        if blocking:
            assert done, f"{entry} ({what}): documented as blocking, returned with its stream still busy"
        else:
            assert not done, f"{entry} {label} ({what}): waited for its stream; the header promises it only enqueues"


def _seq_null(nat, si):
    if si not in _SEQ_NULL:
        run, out = _seq_run(nat, si)
        _seq_steps(run, False, "null stream")
        _SEQ_NULL[si] = out
    return _SEQ_NULL[si]


def _seq_same(got, want, what):
    assert got["tickets_zero"] and want["tickets_zero"], what
    for name in want:
        if name in ("tickets_zero", "lists"):
            continue
        assert wc.same_bits(got[name], want[name]), f"the filtered sequence ({what}): '{name}' differs from the null-stream run"
    assert np.array_equal(got["counts_async"], got["counts"]), what
    for g, n in enumerate(got["counts"]):                            # (what lies behind a list's length is not defined)
        assert np.array_equal(got["lists"][g, :n], want["lists"][g, :n]), (what, g)
        assert (np.diff(got["lists"][g, :n].astype(np.int64)) > 0).all(), (what, g)


def _bmu_on_the_null_stream(nat, inp):
    """dbgsom_bmu of the same rows, norms from dbgsom_row_sqnorms, everything on the null stream -> (idx, dist)"""
    import torch

    from tests import device_abi as da

    true = inp.dev()[0]
    N, d, M = inp.N, inp.d, inp.M
    xx = torch.empty(N, dtype=torch.float64, device="cuda")
    ww = torch.empty(M, dtype=torch.float64, device="cuda")
    idx = torch.empty(N, dtype=torch.int64, device="cuda")
    dist = torch.empty(N, dtype=torch.float64, device="cuda")
    nat.call("dbgsom_row_sqnorms", true["X"].data_ptr(), da.F32, N, d, d, xx.data_ptr(), da.stream())
    nat.call("dbgsom_row_sqnorms", true["W"].data_ptr(), da.F64, M, d, d, ww.data_ptr(), da.stream())
    nat.call("dbgsom_bmu", true["X"].data_ptr(), da.F32, N, d, d, xx.data_ptr(), true["W"].data_ptr(), M, ww.data_ptr(), 1, 0,
             idx.data_ptr(), dist.data_ptr(), da.stream())
    torch.cuda.synchronize()
    return idx.cpu().numpy(), dist.cpu().numpy()


@pytest.mark.parametrize("si", sc.SEQUENCE_SHAPES)
def test_filtered_sequence_behind_a_delay(nat, rig, si):
    """norms, planes, five searches (stateless and hinted, with and without DBGSOM_PRUNE, the refinement on) and the
    readers of their workspace on one non-blocking stream: the one place where the fork and join of the search's side
    streams is exercised from a non-blocking caller"""
    from tests import filter_device as fd

    inp = _seq_inputs(si)
    null = _seq_null(nat, si)
    bmu_idx, bmu_dist = _bmu_on_the_null_stream(nat, inp)
    assert np.array_equal(bmu_idx, inp.ref_idx) and wc.same_bits(bmu_dist, inp.ref_dist)
    for name in ("X", "W"):                                          # the sensitivity control
        _, out = _seq_run(nat, si, keep_decoy=(name,))
        assert any(not wc.same_bits(out[k], null[k]) for k in null if k.startswith("dist:")), name
        if name == "W":                                              # the readers: the gap table is a function of W alone
            assert not wc.same_bits(out["gaps"], null["gaps"])
    run, out = _seq_run(nat, si, rig.stream(0), rig.cycles())
    _seq_steps(run, True, "behind the delay")
    for label, _, _ in sc.search_calls():
        assert np.array_equal(out[f"idx:{label}"], inp.ref_idx), label
        assert wc.same_bits(out[f"dist:{label}"], inp.ref_dist), label
    _seq_same(out, null, "behind the delay")
    fd.check_counts(out["counts"].astype(np.int64), inp.N, inp.M, None, inp.ref_idx)
    fd.check_refine_counts(out["refine_counts"], inp.N, inp.M)


@pytest.mark.parametrize("order", ["AB", "BA"])
def test_two_filtered_sequences_on_two_streams_at_once(nat, rig, order):
    """the thread-local helpers of the filtered search (side streams, events, the stage timer) are shared by every raw
    call of the thread: two sequences of different shapes on two streams, queued alternately"""
    import torch

    shape = dict(zip("AB", sc.SEQUENCE_SHAPES))
    streams = {"A": rig.stream(1), "B": rig.stream(2)}
    null = {tag: _seq_null(nat, shape[tag]) for tag in order}
    runs = {tag: sc.FilteredRun(nat, _seq_inputs(shape[tag])) for tag in order}
    torch.cuda.synchronize()
    for tag in order:
        runs[tag].launch_searches(streams[tag], rig.cycles())
    for tag in order:
        runs[tag].read(streams[tag], rig.cycles())
    for tag in order:
        out = runs[tag].finish()
        _seq_steps(runs[tag], True, f"{tag} of {order}")
        _seq_same(out, null[tag], f"{tag} of {order}")


# ---- the anchored forms: the run table, both searches, their readers ------------------------------------------------------
_ANCHORED = {}


def _anchored_inputs():
    if "inp" not in _ANCHORED:
        _ANCHORED["inp"] = sc.AnchoredInputs()
    return _ANCHORED["inp"]


def _anchored_run(nat, stream=None, cycles=0, keep_decoy=()):
    import torch

    run = sc.AnchoredRun(nat, _anchored_inputs())
    torch.cuda.synchronize()
    run.launch_searches(stream, cycles, keep_decoy).read(stream, cycles)
    return run, run.finish()


def _anchored_null(nat):
    if "null" not in _ANCHORED:
        run, out = _anchored_run(nat)
        _seq_steps(run, False, "null stream")
        _ANCHORED["null"] = out
    return _ANCHORED["null"]


def _anchored_same(got, want, what):
    assert got["tickets_zero"] and want["tickets_zero"], what
    for name in want:
        if name != "tickets_zero":
            assert wc.same_bits(got[name], want[name]), f"the anchored sequence ({what}): '{name}' differs from the null-stream run"


def test_anchored_sequence_behind_a_delay(nat, rig):
    """dbgsom_anchor_runs_build, dbgsom_bmu_filtered_anchored and dbgsom_bmu_filtered_anchor_runs on one non-blocking stream
    and a workspace zeroed there, then their readers: winners and distances are the chain's and dbgsom_bmu_filtered's,
    the run table and the bounds pass the checks of tests/test_gpu_anchor_mark_device.py"""
    from tests import test_gpu_anchor_mark_device as tamd

    inp = _anchored_inputs()
    null = _anchored_null(nat)
    for name, seen_in in (("X", "dist:anchored"), ("W", "dist:anchor_runs"), ("anchors", "run_R")):   # the sensitivity control
        _, out = _anchored_run(nat, keep_decoy=(name,))
        assert not wc.same_bits(out[seen_in], null[seen_in]), name
        if name == "anchors":                                        # the readers see it: the bounds are the anchors'
            assert not wc.same_bits(out["low"], null["low"])
    run, out = _anchored_run(nat, rig.stream(0), rig.cycles())
    _seq_steps(run, True, "behind the delay")
    for label in ("anchored", "anchor_runs"):
        assert np.array_equal(out[f"idx:{label}"], inp.ref_idx), label
        assert wc.same_bits(out[f"dist:{label}"], inp.ref_dist), label
    _anchored_same(out, null, "behind the delay")
    got = {"Xs": inp.host["X"], "Wp": inp.host["W"][:inp.M], "anchors": inp.host["anchors"], "aof": inp.host["anchor_of"],
           "order": inp.host["order"], "xx": out["xx"], "run_start": out["run_start"], "anchor": out["run_anchor"],
           "R": out["run_R"], "xx_max": out["run_xx"], "low": out["low"], "up": out["up"], "aseed": out["aseed"]}
    tamd.check_table(got)
    tamd.check_bounds(got)
    assert (out["aseed"] >= 0).all() and (out["aseed"] < inp.M).all() and max(int(v) for v in out["handed"]) <= run.nb


@pytest.mark.parametrize("order", ["AB", "BA"])
def test_anchored_and_filtered_sequences_on_two_streams_at_once(nat, rig, order):
    """the anchored forms share the thread-local helpers and the launch attributes of the plain filtered search: one of
    each on two streams, queued alternately"""
    import torch

    null = {"A": _anchored_null(nat), "B": _seq_null(nat, sc.SEQUENCE_SHAPES[1])}
    runs = {"A": sc.AnchoredRun(nat, _anchored_inputs()), "B": sc.FilteredRun(nat, _seq_inputs(sc.SEQUENCE_SHAPES[1]))}
    streams = {"A": rig.stream(1), "B": rig.stream(2)}
    torch.cuda.synchronize()
    for tag in order:
        runs[tag].launch_searches(streams[tag], rig.cycles())
    for tag in order:
        runs[tag].read(streams[tag], rig.cycles())
    for tag in order:
        out = runs[tag].finish()
        _seq_steps(runs[tag], True, f"{tag} of {order}")
        (_anchored_same if tag == "A" else _seq_same)(out, null[tag], f"{tag} of {order}")


# ---- D. the stage timers ------------------------------------------------------------------------------------------------
def _stage_times(ms5, outer_ms, what):
    times = list(ms5)
    print(f"{what}: stages {['%.4f' % t for t in times]} ms, {outer_ms:.4f} ms between the events around the call")
    assert all(np.isfinite(t) and t >= 0.0 for t in times), times
    assert sum(times) <= outer_ms, (times, outer_ms)


def test_filter_stage_timing_on_a_non_blocking_stream(nat, rig):
    import ctypes

    import torch

    lib = nat.load()
    si, label = sc.SEQUENCE_SHAPES[0], "stateless-prune"
    null = _seq_null(nat, si)
    ms5 = (ctypes.c_double * 5)(*[-1.0] * 5)
    try:
        assert lib.dbgsom_filter_timing(1) == 0
        run = sc.FilteredRun(nat, _seq_inputs(si))
        torch.cuda.synchronize()
        run.launch_searches(rig.stream(0), only=(label,))
        assert lib.dbgsom_bmu_filtered_stage_ms(ms5) == 0, lib.dbgsom_last_error()
        out = run.finish()
        a, b = run.events[("search", label)]
        _stage_times(ms5, a.elapsed_time(b), "dbgsom_bmu_filtered")
        assert sum(ms5) > 0.0
        assert all(rc == 0 for _, _, rc, _, _, _ in run.steps)
        for kind in ("idx", "dist"):
            assert wc.same_bits(out[f"{kind}:{label}"], null[f"{kind}:{label}"]), kind
    finally:
        assert lib.dbgsom_filter_timing(0) == 0
    assert lib.dbgsom_bmu_filtered_stage_ms(ms5) != 0               # off: no timed call


def test_sparse_code_stage_timing_on_a_non_blocking_stream(nat, rig):
    import ctypes

    lib = nat.load()
    key = ("dbgsom_sparse_code_workspace_bytes", 1)
    rec = sc.record(key[0])
    case = rec.cases[key[1]]
    null, _ = _null_run(nat, key)
    ms5 = (ctypes.c_double * 5)(*[-1.0] * 5)
    try:
        assert lib.dbgsom_sparse_code_timing(1) == 0
        r = sc.enqueue(nat, rec, case, rig.stream(0))
        out = sc.finish(r)
        assert r.rc == 0 and lib.dbgsom_sparse_code_stage_ms(ms5) == 0
        _stage_times(ms5, r.before.elapsed_time(r.after), "dbgsom_sparse_code")
        assert sum(ms5) > 0.0
        _same(rec, case, out, null, "with the stage timer on")
    finally:
        assert lib.dbgsom_sparse_code_timing(0) == 0
    assert lib.dbgsom_sparse_code_stage_ms(ms5) == 0 and list(ms5) == [0.0] * 5
