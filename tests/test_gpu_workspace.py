"""MI355X: the workspace contract of include/dbgsom_hip.h over the table of tests/workspace_cases.py.  Every entry
runs on a guarded buffer of EXACTLY the bytes its size function promised (tests/device_abi.py: GuardedWorkspace),
three times: the body zero-filled, filled with 0xFF (every float a NaN, every integer -1), and holding what the
record's other case left there.  The status is 0, the guards and the sentinels around the outputs are intact, the
outputs of the dirty runs are the zero run's bit for bit (the library documents these paths as order-fixed and free
of floating-point atomics), and the zero run passes the gate of the entry's own GPU test.  What production sees --
one buffer that is never cleared, handed to one entry after the other -- is the chain test.  The filtered search,
the one workspace with a contents contract, is honoured as the header words it: zero-filled once, then a sequence of
calls of different shapes and forms, each equal to the same call on a fresh zeroed buffer."""
import numpy as np
import pytest

from tests import device_abi as da
from tests import workspace_cases as wc

pytestmark = pytest.mark.gpu

FILLS = ("zero", "ff", "residue")
CASES = wc.all_cases()
_ZERO = {}          # (size function, case index) -> the outputs of the zero run, shared with the chain


@pytest.fixture(scope="module")
def nat():
    from dbgsom_amd import _native

    _native.load()
    return _native


@pytest.fixture(scope="module")
def o():
    from oracle import som_oracle

    return som_oracle


def _assert_guards(g, used, rec, case, fill):
    front, back = g.intact(used)
    assert front, f"{rec.entry} {case.label} ({fill}): a write in FRONT of the workspace"
    assert back, f"{rec.entry} {case.label} ({fill}): a write BEHIND the {used} bytes {rec.size_fn} promised"


def _call(nat, rec, case, g, used, fill):
    rc, out = wc.run_case(nat, rec, case, g.ptr, used)
    assert rc == 0, f"{rec.entry} {case.label} ({fill}): status {rc}: {nat.load().dbgsom_last_error()}"
    return out


def _zero_run(nat, key):
    if key not in _ZERO:
        rec = wc.records()[key[0]]
        case = rec.cases[key[1]]
        n = rec.nbytes(nat.load(), case)
        g = da.GuardedWorkspace(n)
        g.fill("zero")
        _ZERO[key] = _call(nat, rec, case, g, n, "zero")
        _assert_guards(g, n, rec, case, "zero")
    return _ZERO[key]


@pytest.mark.parametrize("key", CASES, ids=[wc.case_id(k) for k in CASES])
def test_entry_on_a_zeroed_a_poisoned_and_a_used_workspace(nat, key):
    rec = wc.records()[key[0]]
    case = rec.cases[key[1]]
    lib = nat.load()
    n = rec.nbytes(lib, case)
    others = [(c, rec.nbytes(lib, c)) for c in rec.cases if c is not case]
    assert n > 0 and others
    g = da.GuardedWorkspace(max([n] + [m for _, m in others]))
    zero = _zero_run(nat, key)
    for fill in FILLS[1:]:
        g.fill("ff")
        if fill == "residue":                 # the record's other cases have just run here; nothing is cleared behind them
            for other, m in others:
                _call(nat, rec, other, g, m, "in front of the residue run")
        g.reguard(n)
        out = _call(nat, rec, case, g, n, fill)
        _assert_guards(g, n, rec, case, fill)
        for name in case.outputs:
            assert wc.same_bits(out[name], zero[name]), \
                f"{rec.entry} {case.label}: output '{name}' depends on what the workspace held ({fill})"
    case.check(zero, case.inputs())


def test_chain_of_every_entry_on_one_buffer_that_is_never_cleared(nat):
    """table order, one allocation of the largest size: every entry finds what the entries in front of it left (the
    first one 0xFF), as on the context's shared buffers"""
    lib = nat.load()
    recs = wc.records()
    sizes = {key: recs[key[0]].nbytes(lib, recs[key[0]].cases[key[1]]) for key in CASES}
    big = max(sizes.values())
    g = da.GuardedWorkspace(big)
    g.fill("ff")
    for key in CASES:
        rec = recs[key[0]]
        case = rec.cases[key[1]]
        out = _call(nat, rec, case, g, sizes[key], "chain")
        _assert_guards(g, big, rec, case, "chain")
        zero = _zero_run(nat, key)
        for name in case.outputs:
            assert wc.same_bits(out[name], zero[name]), \
                f"{rec.entry} {case.label}: output '{name}' depends on what earlier entries left in the workspace"


def test_filtered_sequence_on_one_zeroed_buffer(nat, o):
    """include/dbgsom_hip.h: the workspace of dbgsom_bmu_filtered is zero-filled ONCE, and its calls leave it ready.
    One guarded buffer, zeroed once; calls that differ in (N, d, M) and in form -- hinted, stateless, DBGSOM_PRUNE with
    and without the re-seeding pass, the probe, the refinement, anchored -- largest workspace first, each given exactly
    its own size: every one equals the same call on a fresh zeroed buffer bit for bit, leaves the tickets zero and
    stays inside its bytes.  (Never 0xFF: that is outside the contract.)"""
    from tests import anchor_seeds as an
    from tests import filter_device as fd
    from tests import test_gpu_anchor_seed_device as tasd
    from tests import test_gpu_filter_device as tfd

    rec = wc.records()["dbgsom_bmu_filtered_workspace_bytes"]
    assert rec.contents == "zero-filled once"
    raw, seeds = tfd._RawCases(nat, o), tasd._SeedRows(nat, o)
    steps = []
    for ci in (3, 10, 39, 2, 8, 45, 1):       # (1000, 48, 300), (129, 16, 129) and (127, 16, 2): hinted and stateless forms
        N, d, M = fd.RAW_SHAPES[fd.RAW_CASES[ci][0]]
        steps.append((tfd._workspace_bytes(nat, N, d, M), "raw", ci))
    for row in ((an.SEED_N, an.PRUNE, (255, 1985, 48, "iso", "f64", "nearest")), an.SEED_EXTRA[1], an.SEED_EXTRA[0]):
        assert row in an.SEED_ROWS
        steps.append((tasd._ws_bytes(nat, row), "anchored", row))
    steps.sort(key=lambda s: -s[0])
    assert len({s[0] for s in steps}) >= 4
    g = da.GuardedWorkspace(steps[0][0])
    g.fill("zero")                            # once
    for n, kind, what in steps:
        run = raw.run if kind == "raw" else seeds.run
        g.reguard(n)                          # (behind this call's bytes; later calls are no larger)
        got = run(what, g.t, g.ptr, n)
        front, back = g.intact(n)
        assert front and back, f"dbgsom_bmu_filtered {kind} {what}: a write {'in front of' if not front else 'behind'} its {n} bytes"
        ws_t, ws = da.workspace(n)
        fresh = run(what, ws_t, ws, n)
        assert got["tickets_zero"] and fresh["tickets_zero"], (kind, what)
        for name in ("idx", "dist", "counts", "aseed", "seed"):
            if name in fresh:
                assert wc.same_bits(got[name], fresh[name]), f"{kind} {what}: '{name}' depends on the calls in front of it"
        if kind == "raw":
            _, _, rd, ri = raw.inputs(fd.RAW_CASES[what][0], fd.RAW_CASES[what][1])
        else:
            _, _, rd, ri = seeds.get(what)
        assert np.array_equal(got["idx"], ri) and np.array_equal(got["dist"], rd), (kind, what)
