"""MI355X: what the anchor seeds leave behind (tests/anchor_seeds.py holds the tables, the references and their
derivations).  Any seed keeps the search exact, so the bit-for-bit cases of tests/test_gpu_anchor_seeds.py pass whatever
anchor_seed_kernel answers; here its answers are read back.

1. dbgsom_bmu_filtered_anchored called raw over a pairwise table of anchor counts, map sizes, feature counts, inputs,
   types and buckets: winners and distances are oracle.som_oracle.bmu_chain's bits; the prototype chosen per anchor
   (dbgsom_bmu_filtered_anchor_seeds) is the np.longdouble arg-min wherever the runner-up is clear of the rounding
   bound, and never worse than the bound; every sample carries the seed of its anchor; the tickets are back at zero;
   and the same bits come out of a fresh workspace and of one shared by every case, forward and reversed.
2. Constructed ties (copies of a row in another 64-block, another wavefront, another accumulator slot): the lowest
   index wins.  Rows with a NaN, an infinity or an overflowing norm are never chosen while a finite row exists.
3. The buckets the context builds (dbgsom_ctx_read_anchors): the anchor rows are the chained strided rows of the stored
   samples bit for bit, every sample sits within 2 eps of its nearest anchor, and the summed distance to the assigned
   anchors is that of the emulated pre-pass."""
import numpy as np
import pytest

import bench
from tests import anchor_seeds as an
from tests import device_abi as da
from tests import golden_inputs as gi
from tests import test_gpu_filter_device as tfd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def o():
    from oracle import som_oracle

    return som_oracle


@pytest.fixture(scope="module")
def nat():
    from dbgsom_amd import _native

    _native.load()
    return _native


# ---- the raw anchored call ------------------------------------------------------------------------------------------
def _stage(nat, inp):
    """tests/test_gpu_filter_device.py's staging (NaN in no column here: ldx = d), with one difference: the device
    copies of W and |w|^2 are whole 64-prototype blocks, zero rows and zero norms behind the M real ones.  The kernel
    loads whole tiles; a tile entry at or beyond M that was compared would then have the key -2 a . w_{M-1}, below
    every real key of an anchor near w_{M-1}, and show as a seed >= M -- not depend on what the allocator left there."""
    import torch

    X, W = inp["X"], inp["W"]
    N, d = X.shape
    M = W.shape[0]
    Mg = (M + 63) // 64 * 64
    dtype = "f64" if X.dtype == np.float64 else "f32"
    xt, xptr = da.stage(X, d, 0, dtype)
    wt = torch.zeros((Mg, d), dtype=torch.float64, device="cuda")
    wt[:M] = da.dev(W)
    xx = tfd._norms(nat, xptr, da.CODE[dtype], N, d, d)
    ww = torch.zeros((Mg,), dtype=torch.float64, device="cuda")
    ww[:M] = tfd._norms(nat, wt.data_ptr(), da.F64, M, d, d)
    pbytes = nat.load().dbgsom_filter_planes_bytes(N, d)
    pt, pptr = tfd._filled(pbytes, 0x7f)
    nat.call("dbgsom_filter_prepare", xptr, da.CODE[dtype], N, d, d, pptr, pbytes, da.stream())
    tfd._sync()
    assert wt.data_ptr() % 256 == 0 and ww.data_ptr() % 256 == 0
    return {"keep": (xt, wt, xx, ww, pt), "x": xptr, "code": da.CODE[dtype], "N": N, "d": d, "ldx": d, "xx": xx.data_ptr(),
            "planes": pptr, "W": wt.data_ptr(), "M": M, "ww": ww.data_ptr()}


def _anchored(nat, st, anchors, anchor_of, order, flags, ws_t, ws, ws_bytes):
    """one dbgsom_bmu_filtered_anchored call -> dict: idx, dist, aseed, seed, whether the tickets are zero behind it"""
    N, d, M, A = st["N"], st["d"], st["M"], anchors.shape[0]
    assert anchors.shape == (A, d) and anchors.dtype == np.float64 and 1 <= A <= an.ANCHOR_MAX
    assert anchor_of.shape == order.shape == (N,) and anchor_of.min() >= 0 and anchor_of.max() < A     # (the gather's bounds)
    assert np.array_equal(np.sort(order), np.arange(N))
    idx, dist = tfd._full((N,), -7, "int64"), tfd._full((N,), float("nan"), "float64")
    a_t, of_t, or_t = da.dev(anchors), da.dev(anchor_of.astype(np.int32)), da.dev(order.astype(np.int32))
    nat.call("dbgsom_bmu_filtered_anchored", st["x"], st["code"], N, d, st["ldx"], st["xx"], st["planes"], st["W"], M, st["ww"],
             a_t.data_ptr(), A, of_t.data_ptr(), or_t.data_ptr(), flags, 0, 0, idx.data_ptr(), dist.data_ptr(), ws, ws_bytes,
             da.stream())
    tfd._sync()
    out = {"idx": idx.cpu().numpy(), "dist": dist.cpu().numpy(), "tickets_zero": not tfd._bytes_at(ws_t, ws, 256).any()}
    aseed, seed = np.full(A, -7, dtype=np.int32), np.full(N, -7, dtype=np.int64)
    nat.call("dbgsom_bmu_filtered_anchor_seeds", ws, N, d, M, A, aseed.ctypes.data, seed.ctypes.data, da.stream())
    out["aseed"], out["seed"] = aseed, seed
    return out


class _SeedRows:
    """inputs, references and staged device copies per row of the table: built once, on first use"""

    def __init__(self, nat, o):
        self.nat, self.o, self.rows = nat, o, {}

    def get(self, row):
        if row not in self.rows:
            inp = an.seed_inputs(row)
            rd, ri = self.o.bmu_chain(inp["X"], inp["W"], 1)
            self.rows[row] = (inp, _stage(self.nat, inp), rd, ri)
        return self.rows[row]

    def run(self, row, ws_t, ws, ws_bytes):
        inp, st, _, _ = self.get(row)
        return _anchored(self.nat, st, inp["anchors"], inp["anchor_of"], inp["order"], row[1], ws_t, ws, ws_bytes)


@pytest.fixture(scope="module")
def seed_rows(nat, o):
    return _SeedRows(nat, o)


def _ws_bytes(nat, row):
    N, _, (A, M, d, *_rest) = row
    return tfd._workspace_bytes(nat, N, d, M)


@pytest.fixture(scope="module")
def shared_runs(nat, seed_rows):
    """every row in ONE workspace, sized for the largest and zero-filled once: table order, then reversed -- behind a
    larger map or more anchors the partial minima and seeds of the earlier call lie in the workspace"""
    sizes = [_ws_bytes(nat, r) for r in an.SEED_ROWS]
    ws_t, ws = da.workspace(max(sizes))
    runs = {}
    n = len(an.SEED_ROWS)
    for tag, seq in (("forward", range(n)), ("reverse", range(n - 1, -1, -1))):
        for ri in seq:
            runs[(tag, ri)] = seed_rows.run(an.SEED_ROWS[ri], ws_t, ws, sizes[ri])
    return runs


@pytest.mark.parametrize("ri", range(len(an.SEED_ROWS)), ids=[an.seed_row_id(r) for r in an.SEED_ROWS])
def test_anchor_seeds_raw(nat, seed_rows, shared_runs, ri):
    row = an.SEED_ROWS[ri]
    N, flags, (A, M, d, kind, dtype, buckets) = row
    inp, _, rd, rix = seed_rows.get(row)
    nbytes = _ws_bytes(nat, row)
    ws_t, ws = da.workspace(nbytes)
    fresh = seed_rows.run(row, ws_t, ws, nbytes)
    ref = an.argmin_reference(inp["anchors"], inp["W"])
    n_eq = an.check_argmin(fresh["aseed"], inp["anchors"], inp["W"], ref)
    print(f"{an.seed_row_id(row)}: {n_eq} of {A} anchors held to the reference arg-min, {len(np.unique(fresh['aseed']))} distinct seeds")
    assert n_eq == A
    for tag, got in (("fresh", fresh), ("forward", shared_runs[("forward", ri)]), ("reverse", shared_runs[("reverse", ri)])):
        assert np.array_equal(got["idx"], rix), (tag, int((got["idx"] != rix).sum()))
        assert np.array_equal(got["dist"], rd), (tag, int((got["dist"] != rd).sum()))
        assert got["tickets_zero"], tag
        assert np.array_equal(got["aseed"], fresh["aseed"]), (tag, "the seeds depend on what the workspace held")
        if not flags & an.PRUNE_RETRY:                   # (the re-seeding pass overwrites the seeds of its workgroups)
            assert np.array_equal(got["seed"], got["aseed"][inp["anchor_of"]].astype(np.int64)), (tag, "gather")


def test_fewer_anchors_behind_more_in_one_workspace(nat, seed_rows, o):
    """256 anchors, then 17 on the same map in the same workspace: the partial minima and seeds of anchors 17 .. 255
    lie behind the second call's"""
    row = (an.SEED_N, an.PRUNE, (256, 1985, 16, "blobs", "f32", "nearest"))
    inp = an.seed_inputs(row)
    rd, rix = o.bmu_chain(inp["X"], inp["W"], 1)
    st = _stage(nat, inp)
    few = np.ascontiguousarray(inp["anchors"][:17])
    few_of = an.nearest_anchor(inp["X"], few)
    few_order = np.argsort(few_of, kind="stable").astype(np.int32)
    nbytes = _ws_bytes(nat, row)
    ws_t, ws = da.workspace(nbytes)
    first = _anchored(nat, st, inp["anchors"], inp["anchor_of"], inp["order"], an.PRUNE, ws_t, ws, nbytes)
    second = _anchored(nat, st, few, few_of, few_order, an.PRUNE, ws_t, ws, nbytes)
    third = _anchored(nat, st, inp["anchors"], inp["anchor_of"], inp["order"], an.PRUNE, ws_t, ws, nbytes)
    ws2_t, ws2 = da.workspace(nbytes)
    fresh = _anchored(nat, st, few, few_of, few_order, an.PRUNE, ws2_t, ws2, nbytes)
    assert an.check_argmin(first["aseed"], inp["anchors"], inp["W"]) == 256
    assert an.check_argmin(second["aseed"], few, inp["W"]) == 17
    assert np.array_equal(second["aseed"], fresh["aseed"]) and np.array_equal(second["aseed"], first["aseed"][:17])
    assert np.array_equal(third["aseed"], first["aseed"])
    for got, of in ((first, inp["anchor_of"]), (second, few_of), (third, inp["anchor_of"]), (fresh, few_of)):
        assert got["tickets_zero"]
        assert np.array_equal(got["idx"], rix) and np.array_equal(got["dist"], rd)
        assert np.array_equal(got["seed"], got["aseed"][of].astype(np.int64))


# ---- 2. ties and rows that are not finite ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", an.TIE_SETS, ids=[f"M{c[0]}-" + "_".join(map(str, c[2])) for c in an.TIE_SETS])
def test_ties_go_to_the_lowest_index(nat, o, case):
    M, d, copies = case
    inp = an.tie_inputs(case)
    rd, rix = o.bmu_chain(inp["X"], inp["W"], 1)
    st = _stage(nat, inp)
    nbytes = tfd._workspace_bytes(nat, an.SEED_N, d, M)
    ws_t, ws = da.workspace(nbytes)
    got = _anchored(nat, st, inp["anchors"], inp["anchor_of"], inp["order"], an.PRUNE, ws_t, ws, nbytes)
    ref = an.argmin_reference(inp["anchors"], inp["W"])
    tied = [a for a in range(an.TIE_A) if int(ref[0][a].argmin()) in copies]      # (argmin: the first of equals)
    assert an.TIE_ANCHOR in tied
    assert an.check_argmin(got["aseed"], inp["anchors"], inp["W"], ref, tied=tied) == an.TIE_A - len(tied)
    assert (got["aseed"][tied] == copies[0]).all(), (got["aseed"][tied], copies)
    assert np.array_equal(got["idx"], rix) and np.array_equal(got["dist"], rd) and got["tickets_zero"]
    assert np.array_equal(got["seed"], got["aseed"][inp["anchor_of"]].astype(np.int64))
    assert not np.isin(rix, copies[1:]).any()            # the search itself never answers a higher copy either


@pytest.mark.parametrize("M,d,every_row", [(130, 48, False), (1985, 16, False), (20, 48, True)])
def test_rows_that_are_not_finite_are_never_seeds(nat, o, M, d, every_row):
    inp = an.bad_inputs(M, d, every_row)
    rd, rix = o.bmu_chain(inp["X"], inp["W"], 1)
    st = _stage(nat, inp)
    nbytes = tfd._workspace_bytes(nat, an.SEED_N, d, M)
    ws_t, ws = da.workspace(nbytes)
    got = _anchored(nat, st, inp["anchors"], inp["anchor_of"], inp["order"], an.PRUNE, ws_t, ws, nbytes)
    if every_row:
        assert not got["aseed"].any() and not got["seed"].any()
    else:
        assert an.finite_rows(inp["W"])[got["aseed"]].all()
    assert an.check_argmin(got["aseed"], inp["anchors"], inp["W"]) == (0 if every_row else an.ANCHOR_MAX)
    assert np.array_equal(got["idx"], rix), int((got["idx"] != rix).sum())
    assert np.array_equal(got["dist"], rd, equal_nan=True), int((got["dist"] != rd).sum())
    assert got["tickets_zero"]
    assert np.array_equal(got["seed"], got["aseed"][inp["anchor_of"]].astype(np.int64))


# ---- 3. the buckets of the context ----------------------------------------------------------------------------------
CTX_MAP, SIGMA = (10, 13), 1.1


def _ctx_samples(N, storage, seed):
    X = bench.make_shard_numpy(N, an.CTX_D, seed)
    if storage == "float64":
        X = X.astype(np.float64) * (1.0 + 2.0 ** -30)
    stored = da.stored(X, {"float32": "f32", "float64": "f64", "bf16": "bf16"}[storage])
    Xp = np.zeros((N, 80))
    Xp[:, :an.CTX_D] = np.asarray(da.widen(stored), dtype=np.float64)
    return X, Xp


def _anchored_backend(X, storage, W0, hop):
    """the epochs tests/test_gpu_anchor_seeds.py runs (the pre-pass's reference epochs, then the anchors), stopped
    behind the first epoch that was seeded from the anchors"""
    from dbgsom_amd.backend import HipBackend

    be = HipBackend(0, algorithm="filtered")
    be.anchor_seeds, be.sweep_planes, be.seed_stride = 1, 4, 4
    be.load(X, storage="bf16" if storage == "bf16" else None)
    tv = float(np.asarray(X, dtype=np.float64).var(axis=0).sum())
    for _ in range(4):
        be.epoch(W0, hop, SIGMA, 1.0 / tv, "compact", True)
        assert be.filter_log[-1][0] == "filtered"
        if be.anchor_searches >= 1:
            break
    return be


@pytest.mark.parametrize("storage", an.CTX_STORAGE)
@pytest.mark.parametrize("N", an.CTX_N)
def test_context_buckets(N, storage):
    """Measured on MI355X (blobs, d = 70, N = 257 / 1000 / 4096): excess of the summed distance to the assigned anchor
    over that to the nearest anchor, device 0.000000 / 0.000564 / 0.000582 for float32 and float64 storage and 0.000000
    / 0.000630 / 0.000486 for bf16; the emulation (r_tilde(levels=1).argmin of tests/test_filter_bound.py) gives the
    same figures to every digit, with not one sample in another bucket; 100 / 94.8 / 92.5 % of the samples (bf16:
    100 / 93.9 / 93.3 %) sit at their exact nearest anchor.  The device may exceed the emulation by half, plus 1e-4:
    its float32 epilogue flips near ties only.  The figures are printed."""
    from dbgsom_amd import _native

    X, Xp = _ctx_samples(N, storage, 2000 + N)
    M = CTX_MAP[0] * CTX_MAP[1]
    rng = np.random.default_rng(3)
    W0 = Xp[rng.choice(N, M, replace=False), :an.CTX_D] + 0.05 * rng.standard_normal((M, an.CTX_D))
    be = _anchored_backend(X, storage, W0, gi.lattice_hops(*CTX_MAP))
    assert be.anchor_state == 1 and be.anchor_builds == 1 and be.anchor_searches >= 1, (be.anchor_state, be.anchor_searches)
    assert be.padded_features == 80
    got = be.read_anchors(aseed=True)
    A = min(256, N)
    rows = an.anchor_rows(N, A)
    if 2 < A < N:
        rows = rows[an.chain(Xp[rows])]
    anchors = got["anchors"]
    assert anchors.shape == (A, 80)
    assert np.array_equal(anchors, Xp[rows]), "the anchors are not the chained strided rows of the stored samples"
    assert not anchors[:, an.CTX_D:].any()
    if N <= 256:
        assert np.array_equal(got["anchor_of"], np.arange(N)) and np.array_equal(got["order"], np.arange(N))
    else:
        aof_em, r, eps = an.emulated_buckets(Xp, anchors)
        an.check_buckets(got["anchor_of"], got["order"], r, eps, A)
        (ex_dev, share_dev), (ex_em, share_em) = an.bucket_quality(r, got["anchor_of"]), an.bucket_quality(r, aof_em)
        print(f"N={N} {storage}: excess device {ex_dev:.6f} emulation {ex_em:.6f}; at the exact nearest anchor "
              f"{100 * share_dev:.2f} % / {100 * share_em:.2f} %; differing buckets {int((got['anchor_of'] != aof_em).sum())}")
        assert ex_dev <= an.QUALITY_FACTOR * ex_em + an.QUALITY_ABS
    # the prototype the last search chose per anchor, against the map it searched
    assert np.array_equal(be.get_weights(1), W0)
    Wp = np.zeros((M, 80))
    Wp[:, :an.CTX_D] = W0
    assert an.check_argmin(got["aseed"], anchors, Wp) == A
    # other samples: nothing to read until the next build
    be.load(_ctx_samples(N, storage, 3000 + N)[0], storage="bf16" if storage == "bf16" else None)
    assert be.anchor_state == 0
    with pytest.raises(_native.DbgsomNativeError) as err:
        be.read_anchors()
    assert err.value.code == -4
    be.release()
