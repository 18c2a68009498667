"""The workspace contract of include/dbgsom_hip.h, one record per `size_t dbgsom_*_bytes(` function of the header
(tests/test_gpu_workspace.py, tests/test_workspace_cpu.py).  No tests in here.

A record names a size function, the entry it sizes the workspace of, the alignment the header documents and the
status a short workspace earns; its cases (at least two per record, of different sizes where the size function has
arguments) are built from the inputs and references the entry's own helper module owns and are compared by the gate
that entry's own GPU test uses.  A case is:

  size_args           the arguments of the size function
  inputs()            {name: host array}, made once
  outputs             {name: (elements, dtype, fill)}: every output goes into a buffer of `fill` with PAD elements of
                      TAIL[dtype] on either side
  args(p, ws, bytes)  the entry's arguments without the stream; p[name] is the address of an input or an output --
                      device addresses on the GPU, never-dereferenced host stand-ins in the CPU file
  pre(nat, p)         device calls that prepare an in/out argument (the fold's state), or None
  check(out, inp)     asserts on the host results
  branches            which launcher branches that touch the workspace the shapes reach

`run_case` is the one place that launches; it needs torch and a GPU."""
import functools

import numpy as np

from tests import device_abi as da

EINVAL, ENOMEM = -1, -3
PAD = 16
TAIL = {"float64": -1234.5, "int64": -7, "int32": -7}

# the two size functions that size a RESULT, not scratch: no contents or residue question arises
EXEMPT = {
    "dbgsom_filter_planes_bytes": "sizes the planes buffer, an output of dbgsom_filter_prepare that later calls read; "
                                  "tests/test_gpu_filter_device.py guards the bytes behind it",
    "dbgsom_anchor_runs_bytes": "sizes the run table, an output of dbgsom_anchor_runs_build that later calls read; "
                                "tests/test_gpu_anchor_mark_device.py guards the bytes behind it",
}


class Case:
    def __init__(self, label, size_args, inputs, outputs, args, check, branches, pre=None):
        self.label, self.size_args, self.outputs, self.args = label, tuple(size_args), outputs, args
        self._inputs, self.check, self.branches, self.pre = inputs, check, branches, pre
        self._cache = None

    def inputs(self):
        if self._cache is None:
            self._cache = {k: np.ascontiguousarray(v) for k, v in self._inputs().items() if v is not None}
        return self._cache


class Record:
    def __init__(self, size_fn, entry, align, cases, bad_size_args, short_status=ENOMEM, contents="any"):
        self.size_fn, self.entry, self.align, self.cases = size_fn, entry, align, cases
        self.bad_size_args, self.short_status, self.contents = bad_size_args, short_status, contents

    def nbytes(self, lib, case):
        return int(getattr(lib, self.size_fn)(*case.size_args))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- launching (GPU) ------------------------------------------------------------------------------------------------
class Staged:
    """the device copies of a case's inputs, made once and read only"""

    def __init__(self, case):
        self.t = {k: da.dev(v if v.size else np.zeros(1, dtype=v.dtype)) for k, v in case.inputs().items()}


@functools.lru_cache(maxsize=None)
def staged(case):
    return Staged(case)


def run_case(nat, rec, case, ws_ptr, ws_bytes):
    """one call of the record's entry on (ws_ptr, ws_bytes) -> (status, {name: host array}); the sentinels around every
    output are checked"""
    import torch

    st = staged(case)
    p = {k: t.data_ptr() for k, t in st.t.items()}
    bufs = {}
    for name, (n, dtype, fill) in case.outputs.items():
        t = torch.full((n + 2 * PAD,), TAIL[dtype], dtype=getattr(torch, dtype), device="cuda")
        t[PAD:PAD + n] = fill
        bufs[name] = t
        p[name] = t.data_ptr() + PAD * t.element_size()
    if case.pre is not None:
        case.pre(nat, p)
    rc = getattr(nat.load(), rec.entry)(*case.args(p, ws_ptr, ws_bytes), da.stream())
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                 # a fault of the device: nothing more is started on it in this session
        import pytest

        pytest.exit(f"{rec.entry} {case.label}: the device faulted ({e})", returncode=3)
    out = {}
    for name, (n, dtype, fill) in case.outputs.items():
        h = bufs[name].cpu().numpy()
        tail = np.array(TAIL[dtype], dtype=h.dtype)
        assert same_bits(h[:PAD], np.full(PAD, tail)) and same_bits(h[PAD + n:], np.full(PAD, tail)), \
            f"{rec.entry} {case.label}: a write outside output '{name}'"
        out[name] = h[PAD:PAD + n].copy()
    return rc, out


# ---- references shared by several records ---------------------------------------------------------------------------
def _norms(A):
    from oracle import som_oracle as o

    return o.row_sqnorms_chain(np.ascontiguousarray(da.widen(A)))


class _Dense:
    """a dense matrix where tests/csr_device.py's check_sums expects a scipy one"""

    def __init__(self, D):
        self.D, self.shape = D, D.shape

    def toarray(self):
        return self.D


def _split_sums(v, M, d):
    return v[:M * d].reshape(M, d), v[M * d:M * d + M], v[M * d + M:M * d + 2 * M], v[M * d + 2 * M:]


# ---- 1. the per-neuron sums -----------------------------------------------------------------------------------------
def _sort_inputs(N, M, weighted, sparse):
    from tests import csr_device as cd
    from tests import epoch_tail as et

    def make():
        X, kw, dist = et.sort_rows(N)
        win = et.sort_winners("mixed_bad", N, M)
        rng = np.random.default_rng(N + M)
        inp = dict(winners=win, kw=kw, dist=dist)
        if weighted:
            sw = rng.integers(0, 4, N).astype(np.float64)
            sw[rng.random(N) < 0.2] = 0.0
            inp["sw"] = sw
        if sparse:
            Xs = cd.sparsify(X, rng)
            inp["indptr"], inp["indices"], inp["data"] = cd.arrays(Xs)
            inp["dense"] = Xs.toarray()
        else:
            inp["X"] = X
        return inp
    return make


def _check_accumulate(M, d):
    from tests import csr_device as cd

    def check(out, inp):
        X = inp["dense"] if "dense" in inp else inp["X"]
        case = (_Dense(X), inp["winners"], inp["kw"], inp["dist"], M, inp.get("sw"), True)
        cd.check_sums(case, *_split_sums(out["sums"], M, d))
        inside = (inp["winners"] >= 0) & (inp["winners"] < M)
        assert not inside.all() and out["status"][0] != 0            # 'mixed_bad': the status word is written
    return check


def _accumulate_case(kind, N, M, branches):
    from tests import epoch_tail as et

    d = et.SORT_D
    outputs = {"sums": (M * (d + 3), "float64", float("nan")), "status": (1, "int32", 77)}
    if kind == "csr":
        def args(p, ws, nbytes):
            return [p["indptr"], p["indices"], p["data"], da.F32, N, d, p["winners"], p["kw"], p.get("sw"), p["dist"], M,
                    p["sums"], p["status"], ws, nbytes]
    else:
        def args(p, ws, nbytes):
            return [p["X"], da.F32, N, d, d, p["winners"], p["kw"]] + ([p["sw"]] if kind == "weighted" else []) + \
                [p["dist"], M, p["sums"], p["status"], ws, nbytes]
    return Case(f"N{N}-M{M}", (N, d, M), _sort_inputs(N, M, kind != "plain", kind == "csr"), outputs, args,
                _check_accumulate(M, d), branches)


_SCATTER1 = "hist + scan + one-wavefront scatter (M > 5120: 4 M bytes of LDS), segsum rows over lanes, finalize NG = 1; " \
            "order, blk, count, seg_start, chunk_pre, slab, ticket and oob all live, status written"
_SCATTER4 = "hist + scan + four-wavefront scatter, finalize in NG = 15 groups + finalize_groups (gslab live), status written"


def _accumulate_record(kind):
    name = {"plain": "dbgsom_accumulate", "weighted": "dbgsom_accumulate_weighted", "csr": "dbgsom_accumulate_csr"}[kind]
    return Record(name + "_workspace_bytes", name, 256,
                  [_accumulate_case(kind, 2049, 5121, _SCATTER1), _accumulate_case(kind, 513, 33, _SCATTER4)],
                  [(-1, 4, 5), (10, 0, 5), (10, 4, 0)])


def _masked_accumulate_case(N, d, M, dtype_name, bad):
    from tests import masked_fit as mf

    def inputs():
        c = mf.accumulate_case(N, d, M, 0.3, dtype_name)
        win = c["winners"].copy()
        if bad:
            win[[3, 100, 256]] = [-1, M, 1 << 40]
        return dict(X=c["X"], winners=win, kw=c["kw"], dist=c["dist"])

    def check(out, inp):
        v = out["sums"]
        Md = M * d
        S, K, A = (v[i * Md:(i + 1) * Md].reshape(M, d) for i in range(3))
        a, E = v[3 * Md:3 * Md + M], v[3 * Md + M:]
        assert not np.isnan(v).any()
        if bad:                                                     # tests/test_gpu_masked_fit.py: status and skipped rows
            assert out["status"][0] != 0 and a.sum() == N - 3
            Sr, Kr, Ar, ar, Er = mf.masked_sums(inp["X"], inp["winners"], inp["kw"], inp["dist"], M)
            assert np.array_equal(A, Ar) and np.array_equal(a, ar)
            np.testing.assert_allclose(S, Sr, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(E, Er, rtol=1e-12)
            return
        (Sr, Kr, Ar, ar, Er), (TS, TK, TE) = mf.accumulate_reference(N, d, M, 0.3, dtype_name)
        assert out["status"][0] == 0 and np.array_equal(A, Ar) and np.array_equal(a, ar) and a.sum() == N
        for label, got, ref, T, n in (("S", S, Sr, TS, A), ("K", K, Kr, TK, A), ("E", E, Er, TE, a)):
            n_ = np.asarray(n, dtype=np.longdouble)
            bound = (n_ + 2) * da.U * T + n_ * da.UL * T
            assert np.all(np.abs(np.asarray(got, dtype=np.longdouble) - ref) <= bound), label

    code = da.F32 if dtype_name == "float32" else da.F64

    def args(p, ws, nbytes):
        return [p["X"], code, N, d, d, p["winners"], p["kw"], p["dist"], M, p["sums"], p["status"], ws, nbytes]
    return Case(f"N{N}-d{d}-M{M}-{dtype_name}", (N, d, M), inputs,
                {"sums": (M * (3 * d + 2), "float64", float("nan")), "status": (1, "int32", 77)}, args, check,
                "bucket sort of accumulate.hip in front (its blk, count, seg_start, chunk_pre, ticket, flags), masked "
                "segsum into the slab, finalize" + ("; status written" if bad else " with lists of more than one chunk"))


# ---- 2. smoothing ---------------------------------------------------------------------------------------------------
def _smooth_case(M, d, layout, branches):
    from tests import epoch_tail as et

    def inputs():
        S, K, a, E, hop, W_old = et.smooth_case(M, d)
        return dict(sums=np.concatenate([S.reshape(-1), K, a, E]), hop=hop.astype(np.float32), W_old=W_old)

    def check(out, inp):                                            # tests/test_gpu_epoch_tail_device.py: the parent's bits
        with np.load(et.GOLDEN) as z:
            key = et.smooth_key(M, d, layout)
            assert same_bits(out["W_new"].reshape(M, d), z[key + "_W"]) and same_bits(out["chg"], z[key + "_chg"].reshape(1))

    def args(p, ws, nbytes):
        return [p["sums"], M, d, p["hop"], et.SIGMA, {"compact": 0, "aligned": 1}[layout], p["W_old"], p["W_new"], p["chg"],
                ws, nbytes]
    return Case(f"M{M}-d{d}-{layout}", (M, d), inputs,
                {"W_new": (M * d, "float64", float("nan")), "chg": (1, "float64", float("nan"))}, args, check, branches)


def _smooth_masked_case(M, d):
    from tests import masked_fit as mf

    def inputs():
        S, K, A, a, E, hop, W_old, sigma = mf.smooth_case(M, d)
        return dict(sums=np.concatenate([S.reshape(-1), K.reshape(-1), A.reshape(-1), a, E]), hop=hop.astype(np.float32),
                    W_old=W_old)

    def check(out, inp):                                            # tests/test_gpu_masked_fit.py
        from oracle import som_oracle as o

        S, K, A, a, E, hop, W_old, sigma = mf.smooth_case(M, d)
        want = mf.masked_smooth(S, K, A, hop, sigma, W_old)
        np.testing.assert_allclose(out["W_new"].reshape(M, d), want, rtol=mf.W_RTOL, atol=mf.W_ATOL)
        np.testing.assert_allclose(out["chg"][0], o.change_total(W_old, want), rtol=1e-10)

    def args(p, ws, nbytes):
        return [p["sums"], M, d, p["hop"], 1.3, p["W_old"], p["W_new"], p["chg"], ws, nbytes]
    return Case(f"M{M}-d{d}", (M, d), inputs,
                {"W_new": (M * d, "float64", float("nan")), "chg": (1, "float64", float("nan"))}, args, check,
                f"centres, both products and the change norm of the masked form; split-K pieces: {da.gemm_splits(M, d)}")


# ---- 3. reductions --------------------------------------------------------------------------------------------------
def _sum_case(n):
    def inputs():
        return dict(v=np.random.default_rng(n).normal(size=n) * 3.0)

    @functools.lru_cache(maxsize=None)
    def exact():
        return da.exact_sum(inputs()["v"])

    def check(out, inp):                                            # tests/test_gpu_device_abi.py
        from fractions import Fraction

        ref, T = exact()
        assert abs(Fraction(float(out["out"][0])) - ref) <= n * Fraction(da.U) * T

    return Case(f"n{n}", (), inputs, {"out": (1, "float64", float("nan"))},
                lambda p, ws, nbytes: [p["v"], n, p["out"], ws, nbytes], check,
                "1024 partial sums in the workspace, every workgroup with more than one trip of its 256 threads"
                if n > 262144 else "1024 partial sums in the workspace, most workgroups with one trip")


def _wcol_case(N, d, dtype, with_mean):
    def inputs():
        rng = np.random.default_rng(N + d + 1)
        vals = (rng.normal(size=(N, d)) * 2.0 + 0.5).astype(np.float32)
        X = da.stored(vals, dtype)
        w = rng.integers(0, 4, N).astype(np.float64) * rng.uniform(0.1, 2.5, N)
        mean = np.asarray(X, dtype=np.float64).mean(axis=0).astype(np.float32).astype(np.float64)
        return dict(X=X, w=w, mean=mean)

    def check(out, inp):                                            # tests/test_gpu_device_abi.py
        L = np.longdouble
        Xw = np.asarray(inp["X"], dtype=np.float64)
        base = (Xw.astype(L) - inp["mean"].astype(L)) ** 2 if with_mean else Xw.astype(L)
        terms = inp["w"].astype(L)[:, None] * base
        ref, T = terms.sum(axis=0), np.abs(terms).sum(axis=0)
        assert np.all(np.abs(out["out"].astype(L) - ref) <= (N + 2) * da.U * T + 2 * N * da.UL * T)

    return Case(f"N{N}-d{d}-{dtype}", (d,), inputs, {"out": (d, "float64", float("nan"))},
                lambda p, ws, nbytes: [p["X"], da.CODE[dtype], N, d, d, p["w"], p["mean"] if with_mean else None, p["out"],
                                       ws, nbytes], check,
                "row-block partials of every column in the workspace, summed in block order"
                + (", squared deviations from the mean" if with_mean else ""))


def _covariance_case(N, d, p_, dtype, branches):
    from tests import linear_init as li

    def inputs():
        X, mean, V = li.raw_case(N, d, p_, "true", dtype)[:3]
        return dict(X=X, mean=mean, V=V)

    def check(out, inp):                                            # tests/test_gpu_linear_init.py
        _, _, _, Z, s, zb, sb = li.raw_case(N, d, p_, "true", dtype)
        assert li.within(out["Z"].reshape(d, p_), Z, zb)[0] and li.within(out["colsum"], s, sb)[0]

    return Case(f"N{N}-d{d}-p{p_}-{dtype}", (N, d, p_), inputs,
                {"Z": (d * p_, "float64", -7.25), "colsum": (d, "float64", -7.25)},
                lambda p, ws, nbytes: [p["X"], da.CODE[dtype], N, d, d, p["mean"], p["V"], p_, p["Z"], p["colsum"], ws,
                                       nbytes], check, branches)


# ---- 4. the direct-form searches ------------------------------------------------------------------------------------
def _bmu_masked_case(N, d, M, dtype_name, k, branches):
    from tests import test_missing_cpu as tm

    def inputs():
        X, W, _ = tm.case(N, d, M, 0.3, dtype_name)
        return dict(X=X, W=W)

    def check(out, inp):                                            # tests/test_gpu_missing.py
        want_dist, want_idx = tm.winners_of(tm.case(N, d, M, 0.3, dtype_name)[2], k)
        assert np.array_equal(out["idx"].reshape(want_idx.shape), want_idx)
        np.testing.assert_allclose(out["dist"].reshape(want_dist.shape), want_dist, rtol=tm.RTOL, atol=0)

    code = da.F32 if dtype_name == "float32" else da.F64
    return Case(f"N{N}-d{d}-M{M}-{dtype_name}-k{k}", (code, N, d, M), inputs,
                {"idx": (N * k, "int64", -7), "dist": (N * k, "float64", float("nan"))},
                lambda p, ws, nbytes: [p["X"], code, N, d, d, p["W"], M, d, k, p["idx"], p["dist"], ws, nbytes], check,
                branches)


def _bmu_manhattan_case(dtype, N, d, M, k, branches):
    from tests import manhattan as mh

    def inputs():
        X, W = mh.raw_case(dtype, N, d, M)
        return dict(X=X, W=W)

    def check(out, inp):                                            # tests/test_gpu_manhattan.py: bit for bit
        want_dist, want_idx = mh.l1_select(mh.raw_reference(dtype, N, d, M), k)
        assert np.array_equal(out["idx"].reshape(N, k), want_idx) and same_bits(out["dist"].reshape(N, k), want_dist)

    return Case(f"{dtype}-N{N}-d{d}-M{M}-k{k}", (da.CODE[dtype], N, d, M), inputs,
                {"idx": (N * k, "int64", -77), "dist": (N * k, "float64", -77.0)},
                lambda p, ws, nbytes: [p["X"], da.CODE[dtype], N, d, d, p["W"], M, d, k, p["idx"], p["dist"], ws, nbytes],
                check, branches)


# ---- 5. the k nearest prototypes ------------------------------------------------------------------------------------
def _pd_case(i):
    from tests import prototype_distances as pd

    case = pd.CASES[i]
    dtype, N, M, d = case[:4]
    assert dtype == "f32"
    return case, N, M, d


def _kneighbors_case(i, k, slab, branches):
    from tests import kneighbors as kn
    from tests import prototype_distances as pd

    case, N, M, d = _pd_case(i)

    def inputs():
        X, W, _ = pd.case_data(case)
        return dict(X=X, W=W, xx=_norms(X), ww=_norms(W))

    def check(out, inp):                                            # tests/test_gpu_kneighbors.py
        X, W, D = pd.case_data(case)
        want = kn.topk_oracle(X, W, k, D)
        assert np.array_equal(out["idx"].reshape(N, k), want)
        assert same_bits(out["dist"].reshape(N, k), np.take_along_axis(D, want, axis=1))

    return Case(f"N{N}-M{M}-d{d}-k{k}-slab{slab}", (N, M, slab), inputs,
                {"idx": (N * k, "int64", kn.IDX_SENTINEL), "dist": (N * k, "float64", pd.SENTINEL)},
                lambda p, ws, nbytes: [p["X"], da.F32, N, d, d, p["xx"], p["W"], M, p["ww"], k, slab, p["idx"], p["dist"],
                                       ws, nbytes], check, branches)


def _kneighbors_cosine_case(i, k, slab, branches):
    from tests import cosine as cs
    from tests import kneighbors as kn
    from tests import prototype_distances as pd

    case, N, M, d = _pd_case(i)

    def inputs():
        X, W, _ = cs.case_data(case)
        return dict(X=X, W=W, u=cs.inv_norms(cs.sqnorm_chain(X)), v=cs.inv_norms(cs.sqnorm_chain(W)))

    def check(out, inp):                                            # tests/test_gpu_cosine.py: bit for bit
        want_dist, want_idx = cs.select(cs.case_data(case)[2], k)
        assert np.array_equal(out["idx"].reshape(N, k), want_idx) and same_bits(out["dist"].reshape(N, k), want_dist)

    return Case(f"N{N}-M{M}-d{d}-k{k}-slab{slab}", (N, M, slab), inputs,
                {"idx": (N * k, "int64", -77), "dist": (N * k, "float64", pd.SENTINEL)},
                lambda p, ws, nbytes: [p["X"], da.F32, N, d, d, p["u"], p["W"], M, p["v"], k, slab, p["idx"], p["dist"],
                                       ws, nbytes], check, branches)


def _kneighbors_masked_case(N, d, M, dtype_name, k, slab, branches):
    from tests import kneighbors as kn
    from tests import prototype_distances as pd
    from tests import test_missing_cpu as tm

    def inputs():
        X, W, _ = tm.case(N, d, M, 0.3, dtype_name)
        return dict(X=X, W=W)

    def check(out, inp):                                            # tests/test_gpu_kneighbors.py
        D = tm.case(N, d, M, 0.3, dtype_name)[2]
        idx = out["idx"].reshape(N, k)
        assert np.array_equal(idx, np.argsort(D, axis=1, kind="stable")[:, :k])
        np.testing.assert_allclose(out["dist"].reshape(N, k), np.take_along_axis(D, idx, axis=1), rtol=tm.RTOL, atol=0.0)

    code = da.F32 if dtype_name == "float32" else da.F64
    return Case(f"N{N}-d{d}-M{M}-{dtype_name}-k{k}-slab{slab}", (code, N, d, M, slab), inputs,
                {"idx": (N * k, "int64", kn.IDX_SENTINEL), "dist": (N * k, "float64", pd.SENTINEL)},
                lambda p, ws, nbytes: [p["X"], code, N, d, d, p["W"], M, d, k, slab, p["idx"], p["dist"], ws, nbytes],
                check, branches)


def _kneighbors_manhattan_case(dtype, N, d, M, k, slab, branches):
    from tests import manhattan as mh

    def inputs():
        X, W = mh.raw_case(dtype, N, d, M)
        return dict(X=X, W=W)

    def check(out, inp):                                            # tests/test_gpu_manhattan.py: bit for bit
        want_dist, want_idx = mh.l1_select(mh.raw_reference(dtype, N, d, M), k)
        assert np.array_equal(out["idx"].reshape(N, k), want_idx) and same_bits(out["dist"].reshape(N, k), want_dist)

    return Case(f"{dtype}-N{N}-d{d}-M{M}-k{k}-slab{slab}", (da.CODE[dtype], N, d, M, slab), inputs,
                {"idx": (N * k, "int64", -77), "dist": (N * k, "float64", -77.0)},
                lambda p, ws, nbytes: [p["X"], da.CODE[dtype], N, d, d, p["W"], M, d, k, slab, p["idx"], p["dist"], ws,
                                       nbytes], check, branches)


# ---- 6. the folds down the columns ----------------------------------------------------------------------------------
def _topk_cols_case(N, M, k, kind, branches):
    from tests import exemplars as ex

    case, row0 = (N, M, k, kind), 11

    def inputs():
        return dict(R=ex.cols_matrix(case), owner=ex.cols_owner(case))

    def pre(nat, p):
        nat.call("dbgsom_topk_cols_init", p["state_r"], p["state_i"], M, k, da.stream())

    def check(out, inp):                                            # tests/test_gpu_exemplars.py: bit for bit
        r, i = ex.topk_cols_oracle(inp["R"], k, inp.get("owner"), row0=row0)
        assert same_bits(out["state_r"].reshape(M, k), r) and np.array_equal(out["state_i"].reshape(M, k), i)

    return Case(f"N{N}-M{M}-k{k}-{kind}", (N, M, k), inputs,
                {"state_r": (M * k, "float64", ex.SENTINEL), "state_i": (M * k, "int64", ex.IDX_SENTINEL)},
                lambda p, ws, nbytes: [p["R"], N, M, M, p.get("owner"), row0, k, p["state_r"], p["state_i"], ws, nbytes],
                check, branches, pre=pre)


def _exemplars_case(i, k, own_cell, slab, branches):
    from tests import exemplars as ex
    from tests import prototype_distances as pd

    case, N, M, d = _pd_case(i)

    def inputs():
        X, W, _ = pd.case_data(case)
        return dict(X=X, W=W, xx=_norms(X), ww=_norms(W))

    def check(out, inp):                                            # tests/test_gpu_exemplars.py: bit for bit
        dist, idx = ex.case_reference(case, k, bool(own_cell))
        assert same_bits(out["dist"].reshape(M, k), np.asarray(dist)) and np.array_equal(out["idx"].reshape(M, k), idx)

    return Case(f"N{N}-M{M}-d{d}-k{k}-own{own_cell}-slab{slab}", (N, M, k, slab), inputs,
                {"idx": (M * k, "int64", ex.IDX_SENTINEL), "dist": (M * k, "float64", ex.SENTINEL)},
                lambda p, ws, nbytes: [p["X"], da.F32, N, d, d, p["xx"], p["W"], M, p["ww"], k, own_cell, slab, p["idx"],
                                       p["dist"], ws, nbytes], check, branches)


def _range_counts_case(i, n_radii, slab, branches):
    from tests import density as dn
    from tests import prototype_distances as pd

    case, N, M, d = _pd_case(i)

    def inputs():
        X, W, _ = pd.case_data(case)
        return dict(X=X, W=W, xx=_norms(X), ww=_norms(W), thr=np.asarray(dn.case_reference(case, n_radii)[1]))

    def check(out, inp):                                            # tests/test_gpu_density.py: exact
        assert np.array_equal(out["counts"].reshape(M, n_radii), dn.case_reference(case, n_radii)[2])

    return Case(f"N{N}-M{M}-d{d}-n{n_radii}-slab{slab}", (N, M, slab), inputs,
                {"counts": (M * n_radii, "int64", dn.SENTINEL)},
                lambda p, ws, nbytes: [p["X"], da.F32, N, d, d, p["xx"], p["W"], M, p["ww"], p["thr"], n_radii, slab,
                                       p["counts"], ws, nbytes], check, branches)


# ---- 7. graphs ------------------------------------------------------------------------------------------------------
def _geodesics_case(name, branches):
    from tests import combined_error as ce

    M, edges, lengths, sources = ce.GRAPHS[name]()                  # (the reference rows only where they are compared)
    E, S = len(edges), (M if sources is None else len(sources))

    def inputs():
        return dict(edges=np.asarray(edges, dtype=np.int32), lengths=np.asarray(lengths, dtype=np.float64),
                    sources=None if sources is None else np.asarray(sources, dtype=np.int32))

    def check(out, inp):                                            # tests/test_gpu_combined_error.py: bit for bit
        assert same_bits(out["G"].reshape(S, M), np.asarray(ce.graph(name)[4]))

    return Case(name, (M, E), inputs, {"G": (S * M, "float64", ce.SENTINEL)},
                lambda p, ws, nbytes: [p["edges"], p["lengths"], E, M, p.get("sources"), S, p["G"], M, ws, nbytes], check,
                branches)


def _topofn_case(name, full, branches):
    from tests import topofn_device as td

    idx2, xy, M = td.CASES[name]()                                  # (the reference only where it is compared)
    n, n_pos = len(idx2), td.n_pos_of(xy)

    def inputs():
        return dict(idx2=np.asarray(idx2, dtype=np.int64), xy=np.asarray(xy, dtype=np.int32))

    def check(out, inp):                                            # tests/test_gpu_topofn_device.py: exact
        wp, wn, WD = td.reference(inp["idx2"], inp["xy"], M)
        assert np.array_equal(out["hist_pos"], wp) and np.array_equal(out["hist_neg"], wn)
        if full:
            assert np.array_equal(out["D"].reshape(M, M), WD)

    outputs = {"hist_pos": (n_pos, "int64", -7), "hist_neg": (M + 1, "int64", -7)}
    if full:
        outputs["D"] = (M * M, "int32", -7)
    return Case(f"{name}-{'full' if full else 'histogram'}", (M, int(full)), inputs, outputs,
                lambda p, ws, nbytes: [p["idx2"], n, p["xy"], M, n_pos, p["hist_pos"], p["hist_neg"], p.get("D"), ws,
                                       nbytes], check, branches)


# ---- 8. sparse coding -----------------------------------------------------------------------------------------------
SC_LDS_ROWS = 4           # rows of support 5 beside the all-active rows: the LDS path in the same call
SC_CLASSES = 7


def _sparse_code_case(name, branches):
    from tests import sparse_code_inputs as si

    d, M, s, n, noise, seed = si.CASES[name]
    Nq = n + SC_LDS_ROWS

    @functools.lru_cache(maxsize=None)
    def data():
        W, X, _ = si.case(name)
        X = np.vstack([X, si.plant_queries(si.normalize(W), 5, SC_LDS_ROWS, noise, np.random.default_rng(seed + 77))])
        P = np.abs(np.random.default_rng(11).normal(size=(M, SC_CLASSES)))
        code, iters = si.reference(W, X)
        return W, np.ascontiguousarray(X), P, code, iters

    def inputs():
        W, X, P, _, _ = data()
        return dict(X=X, W=W, P=P)

    def check(out, inp):                                            # tests/test_gpu_sparse_code_paths.py: gates and counters
        _, _, P, ref, iters = data()
        code, cnt = out["code"].reshape(Nq, M), out["counts"]
        assert np.abs(code - ref).max() <= si.GATE[np.dtype(np.float64)]
        raw = ref @ P
        np.testing.assert_allclose(out["proba"].reshape(Nq, SC_CLASSES), raw / raw.sum(axis=1)[:, None], rtol=1e-9, atol=1e-12)
        assert cnt[0] == Nq and cnt[1] == int(iters.sum()) and cnt[2] == int(iters.max())
        assert cnt[7] == n and cnt[8] == M                           # the planted rows overflowed, every prototype active

    return Case(name, (Nq, d, M, 1000), inputs,
                {"code": (Nq * M, "float64", float("nan")), "proba": (Nq * SC_CLASSES, "float64", float("nan")),
                 "counts": (11, "int64", 0)},
                lambda p, ws, nbytes: [p["X"], da.F64, Nq, d, d, p["W"], M, d, 1000, 0, p["P"], SC_CLASSES, p["code"],
                                       p["proba"], p["counts"], ws, nbytes], check, branches)


# ---- 9. the filtered search (the one workspace with a contents contract) ----------------------------------------------
def _filtered_case(si_):
    """a stateless raw call of tests/filter_device.py's shape table: what the CPU file needs (sizes, the refusals).  The
    GPU file runs its own sequence of forms on one zero-filled buffer."""
    from tests import filter_device as fd

    N, d, M = fd.RAW_SHAPES[si_]

    def inputs():
        raise AssertionError("the filtered search is not run through run_case: its workspace has a contents contract")

    def args(p, ws, nbytes):
        return [p["X"], da.F32, N, d, d, p["xx"], p["planes"], p["W"], M, p["ww"], None, None, 0, 0, 0, p["idx"], p["dist"],
                ws, nbytes]
    return Case(f"N{N}-d{d}-M{M}", (N, d, M), inputs, {"idx": (N, "int64", -7), "dist": (N, "float64", float("nan"))}, args,
                None, "see test_filtered_sequence_on_one_zeroed_buffer")


# ---- the table ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def records():
    """-> {size function: Record}, in the header's order"""
    big_rows = 8192 + 17
    recs = [
        _accumulate_record("plain"),
        _accumulate_record("weighted"),
        _accumulate_record("csr"),
        Record("dbgsom_smooth_workspace_bytes", "dbgsom_smooth", 256,
               [_smooth_case(257, 130, "compact", "generic-free product in four split-K pieces, their partials in the "
                             "workspace, centres compacted; the strided change tree in one trip"),
                _smooth_case(1030, 2, "aligned", "eight split-K pieces; more than 1024 rows: the second trip of the "
                             "strided tree of the change norm")],
               [(0, 4), (5, 0)]),
        Record("dbgsom_bmu_filtered_workspace_bytes", "dbgsom_bmu_filtered", 256, [_filtered_case(3), _filtered_case(2)],
               [(0, 16, 130), (10, 16, 0)], contents="zero-filled once"),
        Record("dbgsom_sum_workspace_bytes", "dbgsom_sum_f64", 16, [_sum_case(300001), _sum_case(70001)], []),
        Record("dbgsom_weighted_column_sums_workspace_bytes", "dbgsom_weighted_column_sums", 16,
               [_wcol_case(2049, 65, "f32", True), _wcol_case(513, 37, "f64", False)], [(0,), (-3,)]),
        Record("dbgsom_bmu_masked_workspace_bytes", "dbgsom_bmu_masked", 16,
               [_bmu_masked_case(big_rows, 5, 3, "float32", 2, "Wt, n_obs and the float64 copy of float32 rows; the "
                                 "16-rows-per-workgroup search"),
                _bmu_masked_case(257, 17, 5, "float64", 1, "Wt and n_obs only (float64 rows stay where they are); the "
                                 "4-rows-per-workgroup search")],
               [(0, -1, 4, 5), (0, 10, 0, 5), (0, 10, 4, 0)]),
        Record("dbgsom_kneighbors_workspace_bytes", "dbgsom_kneighbors", 16,
               [_kneighbors_case(3, 5, 0, "one slab of 127 rows x 260 (the whole workspace), K = 8 selection"),
                _kneighbors_case(5, 16, 128, "kneighbors.SLAB_CASE: three slabs of 128, 128 and 44 rows through one slab "
                                 "of M + 1 = 34 columns")],
               [(0, 5, 0), (10, 0, 0)]),
        Record("dbgsom_kneighbors_masked_workspace_bytes", "dbgsom_kneighbors_masked", 16,
               [_kneighbors_masked_case(1000, 64, 129, "float32", 5, 128, "Wt, n_obs and the float64 rows of one slab in "
                                        "front, the slab behind them; eight slabs"),
                _kneighbors_masked_case(257, 17, 5, "float64", 5, 0, "Wt and n_obs in front, one slab")],
               [(0, 0, 4, 5, 0), (0, 10, 0, 5, 0), (0, 10, 4, 0, 0)]),
        Record("dbgsom_topk_cols_workspace_bytes", "dbgsom_topk_cols", 16,
               [_topk_cols_case(20000, 70, 32, "none", "79 segments of 256 rows, 2528 candidates per column: both merge "
                                "stages (segment lists and part lists live)"),
                _topk_cols_case(1000, 129, 16, "random", "8 segments of 128 rows, one merge stage, owners given")],
               [(0, 5, 1), (10, 5, 33), (10, 0, 1)]),
        Record("dbgsom_exemplars_workspace_bytes", "dbgsom_exemplars", 16,
               [_exemplars_case(3, 32, 0, 0, "one slab, no units, K = 32 fold, the state behind the fold's scratch"),
                _exemplars_case(5, 5, 1, 100, "exemplars.SLAB_CASE: three slabs of 100 rows, the units of a slab and their "
                                "distances, K = 8 fold with owners, the state")],
               [(10, 0, 2, 0), (10, 5, 0, 0), (10, 5, 33, 0)]),
        Record("dbgsom_range_counts_workspace_bytes", "dbgsom_range_counts", 16,
               [_range_counts_case(3, 32, 0, "one slab, RB = 32 radii"),
                _range_counts_case(5, 5, 100, "density.SLAB_CASE: three slabs of 100 rows, RB = 8 radii")],
               [(0, 5, 0), (10, 0, 0)]),
        Record("dbgsom_geodesics_workspace_bytes", "dbgsom_geodesics", 256,
               [_geodesics_case("holes16", "the status word; M = 256: vectors of 2 KiB in LDS, 256-lane workgroups, a sheet "
                                "cut in two with four isolated units"),
                _geodesics_case("stride1025", "the status word; M = 8200: vectors above 64 KiB of LDS, 1024-lane "
                                "workgroups, a source list")],
               [(0, 3), (16001, 3), (5, -1)]),
        Record("dbgsom_accumulate_masked_workspace_bytes", "dbgsom_accumulate_masked", 256,
               [_masked_accumulate_case(1000, 130, 300, "float32", False), _masked_accumulate_case(257, 17, 5, "float64", True)],
               [(-1, 4, 5), (10, 0, 5), (10, 4, 0)]),
        Record("dbgsom_smooth_masked_workspace_bytes", "dbgsom_smooth_masked", 256,
               [_smooth_masked_case(300, 130), _smooth_masked_case(37, 17)], [(0, 4), (5, 0)]),
        Record("dbgsom_bmu_manhattan_workspace_bytes", "dbgsom_bmu_manhattan", 16,
               [_bmu_manhattan_case("f32", big_rows, 5, 3, 1, "Wt and the float64 copy of float32 rows; the "
                                    "16-rows-per-workgroup search"),
                _bmu_manhattan_case("f64", 17, 33, 257, 2, "Wt only, two prototype blocks; the 4-rows-per-workgroup search")],
               [(0, -1, 4, 5), (0, 10, 0, 5), (0, 10, 4, 0)]),
        Record("dbgsom_kneighbors_manhattan_workspace_bytes", "dbgsom_kneighbors_manhattan", 16,
               [_kneighbors_manhattan_case("f32", big_rows, 5, 3, 2, 4096, "Wt and the float64 rows of one slab in front, "
                                           "the slab behind; three slabs of 4096, 4096 and 17 rows"),
                _kneighbors_manhattan_case("f64", 17, 33, 257, 5, 0, "Wt in front, one slab of 17 rows x 258")],
               [(0, 0, 4, 5, 0), (0, 10, 0, 5, 0), (0, 10, 4, 0, 0)]),
        Record("dbgsom_kneighbors_cosine_workspace_bytes", "dbgsom_kneighbors_cosine", 16,
               [_kneighbors_cosine_case(3, 5, 0, "one slab of 127 rows x 260"),
                _kneighbors_cosine_case(5, 16, 128, "three slabs of 128, 128 and 44 rows")],
               [(0, 5, 0), (10, 0, 0)]),
        Record("dbgsom_sparse_code_workspace_bytes", "dbgsom_sparse_code", 256,
               [_sparse_code_case("all_active_193", "LDS path (4 rows of support 5), first overflow pass, then the second "
                                  "(3 rows whose 193 prototypes all end active): both lists, both counters, the slots"),
                _sparse_code_case("all_active_65", "LDS path (4 rows) and the first overflow pass (3 rows, 65 active); the "
                                  "second pass finds an empty list")],
               [(-1, 4, 5, 1000), (10, 0, 5, 1000), (10, 4, 0, 1000), (10, 4, 5, -1)], short_status=EINVAL),
        Record("dbgsom_topofn_workspace_bytes", "dbgsom_topofn", 256,
               [_topofn_case("path", True, "full mode, M = 1500: status, edge bitmap, row pointers, lattice neighbours "
                             "and their distances, the column lists"),
                _topofn_case("long_range", False, "histogram mode, M = 1300: the searches stop early")],
               [(0, 1), (-1, 0), (16001, 1)]),
        Record("dbgsom_covariance_apply_workspace_bytes", "dbgsom_covariance_apply", 16,
               [_covariance_case(129, 1025, 8, "f32", "the wide form (d > 1024): column blocks over blockIdx.y, partials of "
                                 "every row share in the workspace"),
                _covariance_case(997, 65, 8, "f32", "the LDS form, one column per thread, several row shares")],
               [(0, 4, 2), (10, 0, 2), (10, 4, 0), (10, 4, 9)]),
    ]
    return {r.size_fn: r for r in recs}


def all_cases(contents="any"):
    """(size function, case index) of every case whose record accepts `contents` on entry"""
    return [(name, i) for name, r in records().items() if r.contents == contents for i in range(len(r.cases))]


# what tests/stream_cases.py shares with this table: the rows of prototype_distances.CASES and the chain norms
pd_case, row_norms = _pd_case, _norms


def case_id(key):
    name, i = key
    return name[len("dbgsom_"):-len("_bytes")].replace("_workspace", "") + ":" + records()[name].cases[i].label
