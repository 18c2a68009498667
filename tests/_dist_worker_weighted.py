"""Worker of tests/test_gpu_sample_weight.py: one rank of a gloo group, every rank a HipBackend on GPU 0
with its row shard and ITS rows' weights (the pattern of tests/_dist_worker_hip.py)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = port
    import torch.distributed as td

    td.init_process_group("gloo", rank=rank, world_size=world)
    from dbgsom_amd import SomClassifier, SomVQ
    from dbgsom_amd.backend import shard_bounds
    from tests import golden_inputs_weighted as giw

    res = {}
    name = "weighted_digits_vq"
    X, _, w = giw.case(name)
    est = SomVQ(**giw.EST_KWARGS[name]).fit(X, sample_weight=w)          # every rank holds X and w
    res.update(fit_weights=est.weights_, fit_labels=est.labels_, fit_qe=est.quantization_error_,
               fit_te=est.topographic_error_, fit_n_iter=est.n_iter_, fit_neurons=np.array(est.neurons_),
               fit_hits=est._extract_values_from_graph("hit_count"),
               fit_threshold=est.growing_threshold_)
    lo, hi = shard_bounds(len(X), rank, world)
    loc = SomVQ(sharded_input=True, **giw.EST_KWARGS[name]).fit(X[lo:hi], sample_weight=w[lo:hi])   # its rows only
    res.update(loc_weights=loc.weights_, loc_labels=loc.labels_, loc_qe=loc.quantization_error_,
               loc_te=loc.topographic_error_, loc_n_iter=loc.n_iter_, loc_neurons=np.array(loc.neurons_))
    name = "weighted_digits_entropy"
    X, y, w = giw.case(name)
    clf = SomClassifier(**giw.EST_KWARGS[name]).fit(X, y, sample_weight=w)
    res.update(clf_weights=clf.weights_, clf_n_iter=clf.n_iter_, clf_neurons=np.array(clf.neurons_),
               clf_label=clf._extract_values_from_graph("label"),
               clf_probabilities=clf._extract_values_from_graph("probabilities"))
    np.savez(out, **res)
    td.barrier()
    td.destroy_process_group()


if __name__ == "__main__":
    main()
