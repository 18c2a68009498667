"""Record tests/golden/epoch_tail_parent.npz: what dbgsom_smooth and one dbgsom_ctx_epoch give on the cases of
tests/epoch_tail.py, from whichever build of the library is loaded.

The file in the repository was recorded on an MI355X from the library of the commit IN FRONT OF the batched tail
kernels (build that commit, then point DBGSOM_LIB at its libdbgsom_hip.so and run this from the tree that has the
cases); tests/test_gpu_epoch_tail_device.py compares the present library with it bit for bit.  Only calls both
commits have are used.

    DBGSOM_LIB=/path/to/parent/libdbgsom_hip.so python tools/record_epoch_tail_golden.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dbgsom_amd import _native as nat  # noqa: E402
from tests import epoch_tail as et  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else et.GOLDEN
    nat.load()
    arrays = {}
    cases = [(M, d, False) for (M, d) in et.SMOOTH_CASES] + [et.SMOOTH_NAN_CASE + (True,)]
    for M, d, nan_row in cases:
        case = et.smooth_case(M, d, nan_row)
        for layout in et.LAYOUTS:
            W, chg = et.smooth_call(nat, case, layout)
            W2, chg2 = et.smooth_call(nat, case, layout)
            assert np.array_equal(W, W2, equal_nan=True) and np.array_equal(chg, chg2, equal_nan=True)
            key = et.smooth_key(M, d, layout, nan_row)
            arrays[key + "_W"], arrays[key + "_chg"] = W, chg
    arrays.update(et.epoch_call(nat))
    assert sorted(arrays) == sorted(et.golden_keys())
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **arrays)
    print("recorded %d arrays from %s into %s (%d bytes)" % (len(arrays), nat.LIB_PATH, out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
