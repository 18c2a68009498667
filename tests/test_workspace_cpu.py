"""CPU: the workspace contract of include/dbgsom_hip.h as far as it shows without a GPU -- the table of
tests/workspace_cases.py covers every size function of the header, the size functions answer 0 to bad arguments, and
every entry refuses a short or a misaligned workspace with a status code.  The pointers handed over are host
stand-ins that are never dereferenced (the pattern of tests/test_sparse_code_cpu.py): a call that got past its checks
would try to launch and come back with DBGSOM_EHIP here, which none of the asserts accepts."""
import re

import numpy as np
import pytest

from dbgsom_amd import _native
from tests import device_abi as da
from tests import workspace_cases as wc

RECORDS = list(wc.records())


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def _header_size_functions():
    with open(_native.HEADER) as f:
        return re.findall(r"^size_t (dbgsom_\w+_bytes)\(", f.read(), re.M)


def test_every_size_function_of_the_header_has_a_record_or_an_exemption():
    names = _header_size_functions()
    assert len(names) >= 24 and len(names) == len(set(names))
    recs = wc.records()
    assert not set(recs) & set(wc.EXEMPT)
    missing = [n for n in names if n not in recs and n not in wc.EXEMPT]
    assert not missing, f"size functions without a record in tests/workspace_cases.py: {missing}"
    assert set(recs) | set(wc.EXEMPT) == set(names), sorted((set(recs) | set(wc.EXEMPT)) - set(names))
    assert set(wc.EXEMPT) == {"dbgsom_filter_planes_bytes", "dbgsom_anchor_runs_bytes"}
    assert all(isinstance(why, str) and len(why) > 20 for why in wc.EXEMPT.values())
    assert list(recs) == [n for n in names if n in recs]            # the header's order
    for name, r in recs.items():
        assert r.align in (16, 256) and r.short_status in (wc.EINVAL, wc.ENOMEM), name
        assert len(r.cases) >= 2 and len({c.label for c in r.cases}) == len(r.cases), name
        assert all(isinstance(c.branches, str) and len(c.branches) > 10 for c in r.cases), name
        assert hasattr(_native.load(), r.entry) and r.entry in _native.SIGNATURES
    # one workspace has a contents contract, and it is the filter's
    assert [n for n, r in recs.items() if r.contents != "any"] == ["dbgsom_bmu_filtered_workspace_bytes"]


def test_guards_intact_sees_one_byte_in_either_guard():
    off, nbytes = 300, 1000
    clean = np.full(off + nbytes + da.GUARD_BACK, da.GUARD_BYTE, dtype=np.uint8)
    for fill in da.BODY_FILL.values():
        clean[off:off + nbytes] = fill
        assert da.guards_intact(clean, off, nbytes) == (True, True)
    for at, want in ((0, (False, True)), (off - 1, (False, True)), (off + nbytes, (True, False)),
                     (clean.size - 1, (True, False))):
        image = clean.copy()
        image[at] ^= 1
        assert da.guards_intact(image, off, nbytes) == want, at
    for at in (off, off + nbytes - 1):                              # the body's own first and last byte are the entry's
        image = clean.copy()
        image[at] = da.GUARD_BYTE ^ 0xFF
        assert da.guards_intact(image, off, nbytes) == (True, True)
    # a shorter use of the same body: what lies behind it counts as guard
    image = clean.copy()
    image[off:off + nbytes] = da.GUARD_BYTE
    image[off:off + 100] = 0
    assert da.guards_intact(image, off, 100) == (True, True)
    image[off + 100] = 0
    assert da.guards_intact(image, off, 100) == (True, False)
    assert da.GUARD_BYTE not in da.BODY_FILL.values() and da.GUARD_FRONT >= 256 and da.GUARD_BACK >= 4096


@pytest.mark.parametrize("name", RECORDS)
def test_size_function_is_zero_for_bad_arguments_and_positive_for_the_cases(lib, name):
    rec = wc.records()[name]
    fn = getattr(lib, name)
    for bad in rec.bad_size_args:
        assert fn(*bad) == 0, bad
    sizes = [rec.nbytes(lib, c) for c in rec.cases]
    assert all(s > 0 for s in sizes), sizes
    if rec.cases[0].size_args:
        assert len(set(sizes)) > 1 or name == "dbgsom_geodesics_workspace_bytes", sizes   # (residue from another size)


class _StandIns:
    """a distinct, 4096-byte aligned host address per argument name; nothing is ever read or written through them"""

    def __init__(self):
        self.buf = np.zeros(1 << 20, dtype=np.uint8)
        self.base = (self.buf.ctypes.data + 4095) // 4096 * 4096
        self.names = {}

    def __getitem__(self, name):
        if name not in self.names:
            self.names[name] = self.base + 4096 * (1 + len(self.names))
            assert self.names[name] + 4096 <= self.buf.ctypes.data + self.buf.size
        return self.names[name]

    def get(self, name, default=None):
        return self[name]


@pytest.mark.parametrize("name", RECORDS)
def test_short_workspace_is_refused_before_anything_is_launched(lib, name):
    rec = wc.records()[name]
    for case in rec.cases:
        p = _StandIns()
        need = rec.nbytes(lib, case)
        rc = getattr(lib, rec.entry)(*case.args(p, p["workspace"], need - 1), None)
        msg = lib.dbgsom_last_error()
        assert rc == rec.short_status, (case.label, rc, msg)
        assert b"workspace" in msg, msg


@pytest.mark.parametrize("name", RECORDS)
def test_misaligned_workspace_is_refused_before_anything_is_launched(lib, name):
    rec = wc.records()[name]
    for case in rec.cases:
        p = _StandIns()
        need = rec.nbytes(lib, case)
        off = 8 if rec.align == 16 else 16                          # aligned for every narrower contract
        rc = getattr(lib, rec.entry)(*case.args(p, p["workspace"] + off, need), None)
        msg = lib.dbgsom_last_error()
        assert rc == wc.EINVAL, (case.label, rc, msg)
        assert b"align" in msg, msg
