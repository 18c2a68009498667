"""Generate ``tests/golden/topofn.npz`` by RUNNING THE REFERENCE's topographic function.

TEST TOOLING.  Runs only in the build container (needs the reference tree, imported through
tools/ref_shim.py as tools/make_golden.py does); what it writes is plain data.  No reference source
text is stored.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_topofn.py

For every case the reference estimator is fitted again on the golden case definition
(tests/golden_inputs.py), its ``weights_`` and ``neurons_`` are checked against the existing
fixture's ``final_weights`` / ``final_neurons``, and then ``topographic_function(Xq)``
(BaseSom.py:955-998) is called.  Recorded per case (keys prefixed ``<case>_``):
    k_pos, k_neg   the two returned arrays
    phi_k, phi     phi(k) for k in [-M - 2, max_dist + 2]
    D              the reference's Floyd-Warshall hop distances as int32, -1 for inf
    nq             the number of query rows (Xq = the case's X[:nq])
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_shim  # noqa: E402

ref_shim.install()

from dbgsom.SomClassifier import SomClassifier  # noqa: E402
from dbgsom.SomVQ import SomVQ  # noqa: E402

from tests import golden_inputs as gi  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "topofn.npz")

# name -> (golden fit case, estimator class, query rows (None = all of X))
CASES = {
    "digits_f64": ("digits_f64", SomVQ, None),
    "digits_f32": ("digits_f32", SomVQ, None),
    "digits_clf": ("digits_clf", SomClassifier, None),
    "grow_blobs_f32": ("grow_blobs_f32", SomVQ, None),
    "blobs_dead": ("blobs_dead", SomVQ, None),
    "ties_int": ("ties_int", SomVQ, None),
    # few queries: many isolated neurons, lattice neighbours without a path between them
    "digits_few": ("digits_f64", SomVQ, 40),
}


def main():
    only = set(sys.argv[1:])
    out = dict(np.load(OUT)) if os.path.exists(OUT) and only else {}
    fitted = {}
    for name, (case, cls, nq) in CASES.items():
        if only and name not in only:
            continue
        t0 = time.time()
        X, y = gi.case_X(case)
        if case not in fitted:
            est = cls(**gi.EST_KWARGS[case]).fit(X, y)
            g = gi.load(case)
            assert np.array_equal(np.asarray(est.weights_), g["final_weights"]), case
            assert np.array_equal(np.array(est.neurons_, dtype=np.int64), g["final_neurons"]), case
            fitted[case] = est
        est = fitted[case]
        Xq = X if nq is None else X[:nq]
        k_pos, k_neg = est.topographic_function(Xq)
        M = len(est.neurons_)
        max_dist = int(est.max_dist_matrix.max())
        ks = np.arange(-M - 2, max_dist + 3, dtype=np.int64)
        phi = np.array([est.phi(int(k)) for k in ks], dtype=np.int64)
        Dr = np.asarray(est._delaunay_maxtrix)
        D = np.where(np.isinf(Dr), -1, Dr).astype(np.int32)
        assert np.array_equal(D.astype(np.float64), np.where(np.isinf(Dr), -1.0, Dr)), name
        out.update({f"{name}_k_pos": np.asarray(k_pos, dtype=np.float64),
                    f"{name}_k_neg": np.asarray(k_neg, dtype=np.float64),
                    f"{name}_phi_k": ks, f"{name}_phi": phi, f"{name}_D": D,
                    f"{name}_nq": np.int64(Xq.shape[0])})
        print(f"{name}: M={M} max_dist={max_dist} unreachable pairs={int((D < 0).sum())} "
              f"({time.time() - t0:.1f} s)", flush=True)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
