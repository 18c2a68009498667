"""CPU: the tables of tests/stream_cases.py as far as they show without a GPU -- every entry of the header that takes
a stream is accounted for, the decoys are legal inputs that differ from the true ones, the words of the `blocks`
column are the header's, and every case hands its entry as many arguments as the prototype has."""
import collections

import numpy as np
import pytest

from dbgsom_amd import _native
from tests import stream_cases as sc
from tests import workspace_cases as wc

CASES = sc.all_keys()


@pytest.fixture(scope="module")
def header():
    with open(_native.HEADER) as f:
        return f.read()


def test_every_entry_that_takes_a_stream_is_accounted_for(header):
    entries = sc.stream_entries(header)
    assert len(entries) >= 64
    covered = sc.covered()
    assert not set(covered) & set(sc.EXEMPT)
    missing = [e for e in entries if e not in covered and e not in sc.EXEMPT]
    assert not missing, f"entries that take a stream and have neither a case, a sequence step nor an exemption: {missing}"
    assert set(covered) | set(sc.EXEMPT) == set(entries), sorted((set(covered) | set(sc.EXEMPT)) - set(entries))
    assert all(isinstance(why, str) and len(why) > 20 for why in sc.EXEMPT.values())
    assert len(sc.EXEMPT) == 0 and len(covered) == len(entries)     # today every entry runs behind the delay
    for name, n in entries.items():                                 # the binding agrees: (..., stream)
        assert len(_native.SIGNATURES[name][1]) == n, name
    steps = set(sc.SEQUENCE_STEPS.values()) | set(sc.ANCHORED_STEPS.values())
    assert len(sc.cases()) == 42 and len(CASES) == 42 + len(sc.plain_records())
    assert len(covered) == 21 + len(sc.PRE_STEPS) + len(steps) + len(sc.plain_records()) and not steps & set(sc.plain_records())
    assert set(sc.BLOCKS) <= set(entries) and set(sc.PRE_STEPS) <= set(entries)


@pytest.mark.parametrize("phrase", sorted(set(sc.BLOCKS.values())))
def test_blocking_phrases_are_the_headers(header, phrase):
    assert " ".join(phrase.split()) in " ".join(header.replace("\n *", " ").split())


@pytest.mark.parametrize("key", CASES, ids=[sc.key_id(k) for k in CASES])
def test_decoys_are_legal_inputs_that_differ(key):
    rec = sc.record(key[0])
    case = rec.cases[key[1]]
    live = sc.live_inputs(case)
    assert live and set(case.inputs()) - set(live) <= set(sc.HOST_ONLY)
    for name, v in live.items():
        assert v.size and (v.dtype.kind in "fi" or name in sc.FIXED), name   # (no storage type travels as bit patterns here)
        dc = sc.decoy(name, v)
        assert dc.shape == v.shape and dc.dtype == v.dtype and dc.flags.c_contiguous, name
        if name in sc.FIXED:
            assert v.dtype.kind in "iu" and np.array_equal(dc, v), name
            continue
        assert not wc.same_bits(dc, v), name
        if v.dtype.kind == "f":                                     # finite wherever the rolled input is: nothing new
            assert np.array_equal(np.isfinite(dc), np.isfinite(np.roll(v, 1, axis=0))), name
            assert np.array_equal(np.isnan(dc), np.isnan(np.roll(v, 1, axis=0))), name
        else:
            assert collections.Counter(dc.reshape(-1).tolist()) == collections.Counter(v.reshape(-1).tolist()), name
    for (entry, label, name), why in sc.UNOBSERVABLE.items():
        if entry == rec.entry and label in (None, case.label):
            assert name in live and name not in sc.FIXED and len(why) > 20


class _StandIns(dict):
    """a distinct stand-in address per argument name; nothing is called with them"""

    def __missing__(self, name):
        self[name] = 4096 * (1 + len(self))
        return self[name]

    def get(self, name, default=None):
        return self[name]


@pytest.mark.parametrize("key", CASES, ids=[sc.key_id(k) for k in CASES])
def test_case_arguments_have_the_arity_of_the_prototype(header, key):
    rec = sc.record(key[0])
    case = rec.cases[key[1]]
    args = case.args(_StandIns(), 1 << 20, 4096)
    assert len(args) + 1 == sc.stream_entries(header)[rec.entry], rec.entry


def test_unobservable_and_blocks_name_entries_of_the_table():
    entries = {sc.record(name).entry: sc.record(name) for name, _ in CASES}
    for entry, label, _ in sc.UNOBSERVABLE:
        assert entry in entries and (label is None or label in [c.label for c in entries[entry].cases])
    assert set(sc.BLOCKS) <= set(entries) | set(sc.SEQUENCE_STEPS.values()) | set(sc.ANCHORED_STEPS.values())
    assert {sc.SEQUENCE_STEPS[r] for r in sc.READERS} == set(sc.BLOCKS) & set(sc.SEQUENCE_STEPS.values())
    assert {sc.ANCHORED_STEPS[r] for r in sc.ANCHORED_READERS} == set(sc.BLOCKS) & set(sc.ANCHORED_STEPS.values())


def test_decoys_of_the_anchored_sequence():
    inp = sc.AnchoredInputs()
    assert (inp.N + 127) // 128 > 1 and inp.M <= 8192 and 1 <= inp.A <= 256
    for name, v in inp.host.items():
        dc = inp.decoys[name]
        assert dc.shape == v.shape and dc.dtype == v.dtype
        if name in sc.ANCHORED_FIXED:
            assert np.array_equal(dc, v)
        else:
            assert np.isfinite(dc).all() and not np.array_equal(dc, v)
    assert not inp.host["W"][inp.M:].any() and not inp.decoys["W"][inp.M:].any()
    assert inp.host["anchor_of"].min() >= 0 and inp.host["anchor_of"].max() < inp.A
    assert np.array_equal(np.sort(inp.host["order"]), np.arange(inp.N))


@pytest.mark.parametrize("si", sc.SEQUENCE_SHAPES)
def test_decoys_of_the_filtered_sequence(si):
    inp = sc.FilteredInputs(si)
    assert (inp.N + 127) // 128 > 1 and inp.M <= 8192               # more than one workgroup; a gap table exists
    for name, v in inp.host.items():
        dc = inp.decoys[name]
        assert dc.shape == v.shape and dc.dtype == v.dtype
        if name in sc.SEQUENCE_FIXED:
            assert np.array_equal(dc, v)
        else:
            assert np.isfinite(dc).all() and not np.array_equal(dc, v)
    assert np.array_equal(inp.host["order"], np.argsort(inp.host["prev"], kind="stable"))
    labels = [c[0] for c in sc.search_calls()]
    assert len(set(labels)) == len(labels) == 5
