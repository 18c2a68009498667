"""Call order: the operations of one ``dbgsom_ctx`` as a table, a stateless reference for each, and seeded walks.

A context caches what the last calls left in HBM -- the winners and their bucket order (the hint), the exact distances
(the hinted pruning bound), the reduced sums, the partition -- and lends a handful of buffers to unrelated calls.  The
contract is that no result depends on the calls that came before.  This module states that contract so that it can be
run: every operation reachable from ``HipBackend`` is one record of ``OPS``, the expected result of a step is what a
FRESH context with ``algorithm="exact"`` returns for that one call (created, loaded with the same rows and attachments,
released: never a long-lived second context, which would share every non-search buffer with the code under test and
mirror a stale-buffer bug), and what a read of cached state must return is kept in a host-side model (``State``) that
only ever takes values from such fresh contexts.

``after`` of a record says what the call does to the five pieces of cached state that gate other calls --
``hint_valid``, ``last_idx_valid`` and the pruning bound (``ResidentSearchState``, csrc/epoch_control.h) and
``part_valid`` and "sums of M readable" (``sumsM``, csrc/engine.hip) -- as ``keeps`` / ``sets`` / ``clears``, each with
the function of engine.hip and the transition (or field) that decides it; tests/test_call_order_cpu.py resolves every
citation to a line and holds the entries of ResidentSearchState against the header itself.

Importable without a GPU: the HIP backend is only touched inside ``hip_backend``."""
import hashlib
import zlib
from dataclasses import dataclass, field

import numpy as np

from tests import anchor_mark as am
from tests import golden_inputs as gi

KEEPS, SETS, CLEARS = "keeps", "sets", "clears"
# the bound only: cleared when the call overwrites the matrix the bound's distances refer to (Wb[distW_buf]) -- the
# resident one behind a frozen epoch, the other one behind an epoch that swapped the buffers
CLEARS_SAME_BUFFER = "clears when it overwrites the bound's matrix"
CLEARS_ON_ATTACH = "clears when weights are attached"       # (set_sample_weight(None) returns before it)
FLAGS = ("hint_valid", "last_idx_valid", "part_valid", "sums", "bound")

MAPS = {130: (10, 13), 256: (16, 16)}
SIGMA_EVOLVING = 0.3        # (tests/test_gpu_lean_anchor_epoch.py: a narrow neighbourhood keeps the clusters' lists short)
SIGMA_FROZEN = 1.1
# the walks: exp(-hop^2 / 2.42) is above zero out to 42 hops, past the diameter of every lattice here, so a unit without
# an active unit in reach -- whose update is 0 / 0: under SIGMA_EVOLVING most of a map that grew by a few rows turns into
# NaN rows within two epochs -- cannot occur.  Maps with rows that are not finite are not what a walk is about.
SIGMA_WALK = 1.1
N_CLASSES = 5
N_TARGETS = 2
ROWS = (1, 131, 700)        # query rows: one row, a partial workgroup behind a full one, several chunks of 128
KS = (1, 2, 5)
GROWTH = (1, 3)


# ----------------------------------------------------------------------------------------------------------------------
# configurations
# ----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Config:
    name: str
    N: int
    d: int
    M: int
    storage: str            # float32 / float64 / bf16
    algorithm: str
    refine: object = None   # None: the engine's default
    kind: str = "dense"     # dense / csr / incomplete

    @property
    def hinted(self):
        return self.algorithm == "filtered_hint" and self.kind == "dense"


# each shape with two settings, each setting on two shapes (the smallest shapes of the filtered forms: M >= 129,
# d no multiple of 16), one CSR resident and one resident with missing entries
CONFIGS = [
    Config("f32-hint", 4096, 48, 130, "float32", "filtered_hint"),
    Config("f32-lean", 4096, 48, 130, "float32", "filtered"),
    Config("f64-hint", 1000, 70, 256, "float64", "filtered_hint"),
    Config("f64-refine", 1000, 70, 256, "float64", "filtered_hint", 1),
    Config("bf16-refine", 4096, 70, 256, "bf16", "filtered_hint", 1),
    Config("bf16-lean", 4096, 70, 256, "bf16", "filtered"),
    Config("csr", 1000, 70, 130, "float32", "filtered_hint", None, "csr"),
    Config("incomplete", 1000, 48, 130, "float64", "filtered_hint", None, "incomplete"),
]
CONFIG = {c.name: c for c in CONFIGS}
DENSE = [c for c in CONFIGS if c.kind == "dense"]
WALK_SEEDS = (0, 1, 2)
WALK_STEPS = 72


def _lattice(M):
    """rows x cols of the lattice whose first M nodes (row-major) a map of M units lies on: a map that grows or
    shrinks by a few rows keeps its neighbours"""
    if M in MAPS:
        return MAPS[M]
    cols = 13 if M < 200 else 16
    return -(-M // cols), cols


def hop_for(M, _cache={}):
    """the lattice of M units (the same object for the same M: the backend re-uploads a hop matrix by identity)"""
    if M not in _cache:
        _cache[M] = np.ascontiguousarray(gi.lattice_hops(*_lattice(M))[:M, :M])
    return _cache[M]


def coords_for(M):
    rows, cols = _lattice(M)
    ii, jj = np.divmod(np.arange(M), cols)
    return np.ascontiguousarray(np.stack([ii, jj], axis=1), dtype=np.int32)


def edges_for(M):
    hop = hop_for(M)
    a, b = np.nonzero(np.triu(hop == 1.0))
    return np.ascontiguousarray(np.stack([a, b], axis=1), dtype=np.int64)


def bf16_round(X32):
    """float32 -> the float32 value of its bfloat16 rounding (nearest even), what the device stores"""
    u = np.ascontiguousarray(X32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u >> np.uint64(16)) & np.uint64(1)) + np.uint64(0x7FFF)
    return ((u + r) & np.uint64(0xFFFF0000)).astype(np.uint32).view(np.float32)


def inputs(cfg, key="call_order"):
    """-> (X as it is loaded, X as a dense float array of the values the device holds, W0)"""
    X, W0 = am.blobs(cfg.N, cfg.d, cfg.M, key)
    if cfg.storage == "float64":
        X = X.astype(np.float64) * (1.0 + 2.0 ** -30)          # (float64 rows that are no float32 values)
    held = bf16_round(X) if cfg.storage == "bf16" else X
    if cfg.kind == "csr":
        from scipy.sparse import csr_matrix

        rng = am.rng_for("csr", cfg.name)
        X = np.where(rng.random(X.shape) < 0.4, X, 0).astype(X.dtype)     # (rows with zeros: CSR rows of unequal length)
        return csr_matrix(X), X, W0
    if cfg.kind == "incomplete":
        rng = am.rng_for("holes", cfg.name)
        X = X.copy()
        X[rng.random(X.shape) < 0.1] = np.nan
        X[:, 0] = np.where(np.isnan(X).all(axis=1), 0.0, X[:, 0])          # (no row without an observed entry)
        return X, X, W0
    return X, held, W0


# ----------------------------------------------------------------------------------------------------------------------
# the model: what the calls so far must have left, taken from fresh contexts only
# ----------------------------------------------------------------------------------------------------------------------
class State:
    def __init__(self, cfg, key="call_order"):
        self.cfg = cfg
        self.X, self.Xd, W0 = inputs(cfg, key)
        self.N = cfg.N
        self.W = W0                     # the current map: what a call that takes host prototypes is handed
        self.resident = None            # Wb[cur], the resident prototypes
        self.labels = self.sw = self.targets = None
        self.winners = None             # idx[icur] while last_idx_valid
        self.sums = None                # (M, read_sums(M)) while sumsM == M
        self.part = None                # (M, W, order, seg_start, counts) while part_valid
        self.sigma = SIGMA_EVOLVING
        tv = float(np.nanvar(np.asarray(self.Xd, dtype=np.float64), axis=0).sum())
        self.total_variance = tv
        self.gamma = 1.0 / tv

    def sigma_for(self, M):
        return self.sigma

    def reload(self, rows):
        """the model behind ``load``: every attachment and everything cached is gone"""
        self.N = rows
        self.resident = self.labels = self.sw = self.targets = self.winners = self.sums = self.part = None

    def rows(self):
        """the resident rows as they are loaded"""
        return self.X if self.N == self.cfg.N else self.X[:self.N]

    def rows_dense(self):
        return self.Xd if self.N == self.cfg.N else self.Xd[:self.N]

    def digest(self):
        h = hashlib.blake2b(digest_size=16)
        h.update(repr((self.cfg.name, self.N, self.sigma)).encode())
        for a in (self.W, self.resident, self.labels, self.sw, self.targets):
            h.update(b"-" if a is None else np.ascontiguousarray(a).tobytes())
        return h.hexdigest()


def query_rows(st, n, key):
    """n rows near the resident ones, in the resident rows' host dtype"""
    rng = am.rng_for("query", st.cfg.name, n, key)
    Xd = np.nan_to_num(np.asarray(st.Xd))
    Q = Xd[rng.integers(0, Xd.shape[0], n)] + 0.25 * rng.standard_normal((n, st.cfg.d))
    return np.ascontiguousarray(Q, dtype=np.float64 if st.cfg.storage == "float64" else np.float32)


def in_form(Q, form, be):
    if form == "csr":
        from scipy.sparse import csr_matrix

        return csr_matrix(Q)
    if form == "device":
        import torch

        return torch.as_tensor(Q, device=f"cuda:{be.device_index}")
    return Q


def host(a):
    """a result as a host array (results of queries on rows in HBM are arrays next to them)"""
    if a is None or isinstance(a, np.ndarray):
        return a
    if hasattr(a, "cpu"):
        return a.cpu().numpy()
    return np.asarray(a)


# ----------------------------------------------------------------------------------------------------------------------
# comparison: bit for bit, every NaN as one (tests/test_gpu_mixture.py)
# ----------------------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        a = np.ascontiguousarray(a, dtype=np.float64)
        return np.where(np.isnan(a), np.nan, a).view(np.uint64)
    return a


def same(got, want):
    """tuples of arrays (or None), bit for bit -> the index of the first that differs, or None"""
    if len(got) != len(want):
        return -1
    for i, (g, w) in enumerate(zip(got, want)):
        if g is None or w is None:
            if g is not w:
                return i
            continue
        g, w = np.asarray(host(g)), np.asarray(host(w))
        if g.shape != w.shape or g.dtype.kind != w.dtype.kind or not np.array_equal(bits(g), bits(w)):
            return i
    return None


def assert_same(got, want, what):
    i = same(got, want)
    assert i is None, f"{what}: result {i} is not the fresh context's"


def assert_oracle_epoch(st, W, out):
    """winners and distances of the NumPy oracle bit for bit, new prototypes to 1e-11"""
    import oracle.som_oracle as o

    oo = o.epoch(np.ascontiguousarray(st.rows_dense()), W, hop_for(len(W)), st.sigma_for(len(W)), st.total_variance, "compact", "chain")
    assert np.array_equal(out[0], oo.winners), "winners differ from the oracle"
    assert np.array_equal(out[1], oo.distances), "distances differ from the oracle"
    np.testing.assert_allclose(out[2], oo.new_weights, rtol=1e-11, atol=1e-12, equal_nan=True)


def oracle_applies(st):
    return st.cfg.kind == "dense" and st.sw is None


# ----------------------------------------------------------------------------------------------------------------------
# the op table
# ----------------------------------------------------------------------------------------------------------------------
def cite(function, token, file="engine.hip"):
    """where an `after` entry is decided: `token` inside `function` of csrc/<file>"""
    return (file, function, token)


def after(**kw):
    """hint_valid / last_idx_valid / part_valid / sums / bound -> (verb, citation); unnamed flags are kept: nothing in
    the call's function names the transition or the field"""
    out = {f: (KEEPS, None) for f in FLAGS}
    for name, v in kw.items():
        out[{"hint": "hint_valid", "idx": "last_idx_valid", "part": "part_valid"}.get(name, name)] = v
    return out


STAGED = cite("stage_weights", "weights_replaced")      # a call that hands over host prototypes overwrites Wb[cur]
ACCUMULATED_PART = cite("accumulate_and_reduce", "part_valid = false")
ACCUMULATED_SUMS = cite("accumulate_and_reduce", "sumsM = M")

AFTER_EPOCH = after(hint=(SETS, cite("dbgsom_ctx_epoch", "sums_made")), idx=(SETS, cite("epoch_bmu", "dense_search_done")),
                    part=(CLEARS, ACCUMULATED_PART), sums=(SETS, ACCUMULATED_SUMS),
                    bound=(SETS, cite("epoch_bmu", "dense_search_done")))
AFTER_EPOCH_CSR = dict(AFTER_EPOCH, last_idx_valid=(SETS, cite("epoch_bmu", "foreign_search_done")),
                       bound=(CLEARS, cite("epoch_bmu", "foreign_search_done")))
AFTER_FOREIGN_EPOCH = after(hint=(CLEARS, cite("metric_epoch", "foreign_search_begun")),
                            idx=(SETS, cite("metric_epoch", "foreign_search_done")), part=(CLEARS, ACCUMULATED_PART),
                            sums=(SETS, ACCUMULATED_SUMS), bound=(CLEARS, cite("metric_epoch", "foreign_search_begun")))
AFTER_UPDATE = after(hint=(CLEARS, cite("dbgsom_ctx_update", "caller_winners_taken")),
                     idx=(SETS, cite("dbgsom_ctx_update", "caller_winners_taken")), part=(CLEARS, ACCUMULATED_PART),
                     sums=(SETS, ACCUMULATED_SUMS), bound=(CLEARS, cite("dbgsom_ctx_update", "foreign_search_begun")))
AFTER_SET_HINT = after(hint=(SETS, cite("dbgsom_ctx_set_hint", "hint_seeded")),
                       idx=(CLEARS, cite("dbgsom_ctx_set_hint", "hint_seeded")),
                       part=(CLEARS, cite("dbgsom_ctx_set_hint", "part_valid = false")),
                       bound=(CLEARS, cite("dbgsom_ctx_set_hint", "hint_seeded")))
AFTER_STAGED = after(bound=(CLEARS_SAME_BUFFER, STAGED))
AFTER_NODE_STATISTICS = after(hint=(CLEARS, cite("dbgsom_ctx_node_statistics", "bucket_order_rewritten")),
                              part=(CLEARS, cite("dbgsom_ctx_node_statistics", "part_valid = false")),
                              sums=(CLEARS, cite("dbgsom_ctx_node_statistics", "sumsM = 0")),
                              bound=(CLEARS_SAME_BUFFER, STAGED))
AFTER_PARTITION = after(part=(SETS, cite("dbgsom_ctx_partition", "part_valid = true")), bound=(CLEARS_SAME_BUFFER, STAGED))
AFTER_LOAD = after(hint=(CLEARS, cite("reset_training_state", "search.reset")), idx=(CLEARS, cite("reset_training_state", "search.reset")),
                   part=(CLEARS, cite("reset_training_state", "part_valid = false")),
                   sums=(CLEARS, cite("reset_training_state", "sumsM = 0")), bound=(CLEARS, cite("reset_training_state", "search.reset")))
KEEPS_ALL = after()

# ops of ResidentSearchState that are exactly one transition: what tests/call_order_flags.cpp is asked about
ONE_TRANSITION = {"set_hint_true": "hint_seeded", "set_hint_random": "hint_seeded",
                  "load_same": "reset", "load_fewer": "reset", "load_more": "reset", "set_weights": "weights_replaced_bound",
                  "update": "caller_winners_taken"}


@dataclass
class Op:
    name: str
    run: object                       # run(be, st, args) -> tuple of arrays, on the context under test
    entries: tuple                    # the dbgsom_ctx_* entries the call reaches
    after: dict = field(default_factory=after)
    needs: tuple = ()                 # what must be attached / resident (documentation; `refusal` decides)
    draw: object = None               # draw(rng, st) -> args
    ref: object = None                # ref(be, st, args) -> (result, extras) on a fresh context; default: run
    refusal: object = None            # refusal(st, args) -> a piece of the error's text, or None
    kinds: tuple = ("dense", "csr")
    reads: bool = False               # reads what an epoch (or a partition) left

    def expected_refusal(self, st, args):
        return self.refusal(st, args) if self.refusal else None


OPS = {}


def op(name, run, entries, **kw):
    OPS[name] = Op(name, run, tuple(entries), **kw)


def _bf16(st):
    return st.cfg.storage == "bf16"


# -- refusals ------------------------------------------------------------------------------------------------------------
def r_complete(st, args=None):
    return "missing entries" if st.cfg.kind == "incomplete" else None


def r_metric(st, args=None):
    if st.cfg.kind == "csr":
        return "CSR residents have no"
    if _bf16(st):
        return "bfloat16 storage has no"
    if st.cfg.kind == "incomplete":
        return "missing entries"
    return "sample weights are attached" if st.sw is not None else None


def r_resident(st, args=None):
    return r_complete(st) or ("no prototypes resident" if st.resident is None else None)


# -- epochs --------------------------------------------------------------------------------------------------------------
def _out(r, Wn):
    return (r.winners, r.distances, Wn, r.errors, r.activations, np.array([r.change_total]))


def _epoch_input(st, form):
    return st.W if form == "host" or st.resident is None else st.resident


def run_epoch(form):
    def run(be, st, args):
        from dbgsom_amd.backend import RESIDENT

        W = _epoch_input(st, form)
        hop = hop_for(len(W))
        if getattr(be, "name", "") != "hip" or form == "host":
            r = be.epoch(W, hop, st.sigma_for(len(W)), st.gamma, "compact", True)
            return _out(r, r.new_weights)
        Wa = W if st.resident is None else RESIDENT
        if form == "frozen":
            r = be.epoch(Wa, hop, st.sigma_for(len(W)), st.gamma, "compact", True, keep_on_device=True, frozen=True)
            return _out(r, be.get_weights(1))
        r = be.epoch(Wa, hop, st.sigma_for(len(W)), st.gamma, "compact", True, keep_on_device=True)
        return _out(r, be.get_weights(0))
    return run


def ref_epoch(form):
    def ref(be, st, args):
        W = _epoch_input(st, form)
        r = be.epoch(W, hop_for(len(W)), st.sigma_for(len(W)), st.gamma, "compact", True)
        out = _out(r, r.new_weights)
        extras = {"winners": r.winners, "W_in": W, "W_out": r.new_weights, "frozen": form == "frozen"}
        if hasattr(be, "read_sums"):
            extras["sums"] = (len(W), be.read_sums(len(W)))
        return out, extras
    return ref


EPOCH_ENTRIES = ("dbgsom_ctx_epoch", "dbgsom_ctx_set_topology", "dbgsom_ctx_epoch_info")
ANY = ("dense", "csr", "incomplete")
op("epoch", run_epoch("host"), EPOCH_ENTRIES, after=AFTER_EPOCH, ref=ref_epoch("host"), refusal=r_complete, needs=("complete rows",),
   kinds=ANY)
op("epoch_resident", run_epoch("resident"), EPOCH_ENTRIES + ("dbgsom_ctx_get_weights",), after=AFTER_EPOCH, ref=ref_epoch("resident"),
   refusal=r_complete, needs=("complete rows",), kinds=ANY)
op("epoch_frozen", run_epoch("frozen"), EPOCH_ENTRIES + ("dbgsom_ctx_get_weights",), after=AFTER_EPOCH, ref=ref_epoch("frozen"), kinds=ANY,
   refusal=r_complete, needs=("complete rows",))
EPOCHS = ("epoch", "epoch_resident", "epoch_frozen")


def _grown(st, how):
    rng = am.rng_for("grow", st.cfg.name, how, len(st.W))
    W = st.W
    if how == "shrink":
        return np.ascontiguousarray(W[:-1])
    if how == "duplicate":
        W = W.copy()
        W[len(W) // 2] = W[0]
        return W
    return np.ascontiguousarray(np.vstack([W, W[-how:] + 0.01 * rng.standard_normal((how, W.shape[1]))]))


def run_growth(be, st, args):
    W = _grown(st, args)
    if getattr(be, "name", "") != "hip":
        r = be.epoch(W, hop_for(len(W)), st.sigma_for(len(W)), st.gamma, "compact", True)
        return _out(r, r.new_weights)
    r = be.epoch(W, hop_for(len(W)), st.sigma_for(len(W)), st.gamma, "compact", True, keep_on_device=True)
    return _out(r, be.get_weights(0))


def ref_growth(be, st, args):
    W = _grown(st, args)
    r = be.epoch(W, hop_for(len(W)), st.sigma_for(len(W)), st.gamma, "compact", True)
    extras = {"winners": r.winners, "W_in": W, "W_out": r.new_weights, "frozen": False}
    if hasattr(be, "read_sums"):
        extras["sums"] = (len(W), be.read_sums(len(W)))
    return _out(r, r.new_weights), extras


op("growth", run_growth, EPOCH_ENTRIES, after=AFTER_EPOCH, ref=ref_growth, refusal=r_complete, kinds=("dense", "csr"),
   draw=lambda rng, st: int(rng.choice(GROWTH)), needs=("complete rows",))
op("shrink", run_growth, EPOCH_ENTRIES, after=AFTER_EPOCH, ref=ref_growth, refusal=r_complete, kinds=("dense", "csr"),
   draw=lambda rng, st: "shrink", needs=("complete rows",))
op("duplicate", run_growth, EPOCH_ENTRIES, after=AFTER_EPOCH, ref=ref_growth, refusal=r_complete, kinds=("dense", "csr"),
   draw=lambda rng, st: "duplicate", needs=("complete rows",))
GROWTHS = ("growth", "shrink", "duplicate")


def _metric_gamma(st, metric):
    """gamma is 1 / the total variance, made for Euclidean distances: an L1 distance is about sqrt(d) times as long, and
    under the Euclidean gamma every sample weight underflows to 0 and the new map is 0 / 0"""
    return st.gamma / st.cfg.d if metric == "manhattan" else st.gamma


def run_metric_epoch(metric):
    def run(be, st, args):
        r = getattr(be, "epoch_" + metric)(st.W, hop_for(len(st.W)), st.sigma_for(len(st.W)), _metric_gamma(st, metric), "compact", True)
        return _out(r, r.new_weights)
    return run


def ref_metric_epoch(metric):
    def ref(be, st, args):
        r = getattr(be, "epoch_" + metric)(st.W, hop_for(len(st.W)), st.sigma_for(len(st.W)), _metric_gamma(st, metric), "compact", True)
        M = len(st.W)
        return _out(r, r.new_weights), {"winners": r.winners, "W_in": st.W, "W_out": r.new_weights, "frozen": False,
                                        "sums": (M, be.read_sums(M))}
    return ref


for _m in ("manhattan", "cosine"):
    op("epoch_" + _m, run_metric_epoch(_m), ("dbgsom_ctx_epoch_" + _m,), after=AFTER_FOREIGN_EPOCH, ref=ref_metric_epoch(_m),
       refusal=r_metric, needs=("dense float32 / float64 rows", "complete rows", "no sample weights"), kinds=ANY)


def run_epoch_masked(be, st, args):
    r = be.epoch_masked(st.W, hop_for(len(st.W)), st.sigma_for(len(st.W)), st.gamma, True)
    return _out(r, r.new_weights)


op("epoch_masked", run_epoch_masked, ("dbgsom_ctx_epoch_masked",), kinds=("incomplete",), needs=("incomplete rows",),
   ref=lambda be, st, args: (lambda out: (out, {"W_out": out[2]}))(run_epoch_masked(be, st, args)))


def _update_args(st):
    """the caller's winners (nearest prototypes by plain NumPy: winners drawn at random would collapse the map onto the
    mean of the rows), sample weights and distances"""
    rng = am.rng_for("update", st.cfg.name, len(st.W))
    X = np.nan_to_num(np.asarray(st.rows_dense(), dtype=np.float64))
    win = ((st.W * st.W).sum(axis=1)[None, :] - 2.0 * (X @ st.W.T)).argmin(axis=1).astype(np.int64)
    return win, 0.5 + 0.5 * rng.random(st.N), rng.random(st.N) + 0.5


def run_update(be, st, args):
    win, kw, dist = _update_args(st)
    return tuple(np.asarray(a) for a in be.update(st.W, hop_for(len(st.W)), st.sigma_for(len(st.W)), kw, win, dist))


def ref_update(be, st, args):
    out = run_update(be, st, args)
    M = len(st.W)
    extras = {"winners": _update_args(st)[0], "W_in": st.W, "W_out": out[0], "frozen": False}
    if hasattr(be, "read_sums"):
        extras["sums"] = (M, be.read_sums(M))
    return out, extras


op("update", run_update, ("dbgsom_ctx_update",), after=AFTER_UPDATE, ref=ref_update, refusal=r_complete, needs=("complete rows",),
   kinds=ANY)


# -- the hint ------------------------------------------------------------------------------------------------------------
def run_set_hint(kind):
    def run(be, st, args):
        M = len(st.W)
        if kind == "true":
            seeds = be.resident_winners(st.W) if st.winners is None or st.winners.max() >= M else st.winners
        else:
            seeds = am.rng_for("hint", st.cfg.name, M).integers(0, M, st.N)
        be.set_hint(seeds, M)
        return ()
    return run


# (a fresh context has nothing to return for set_hint: the calls behind it are the check)
for _k in ("true", "random"):
    op("set_hint_" + _k, run_set_hint(_k), ("dbgsom_ctx_set_hint",) + (("dbgsom_ctx_bmu",) if _k == "true" else ()),
       after=AFTER_SET_HINT, ref=lambda be, st, args: ((), {}), refusal=r_complete, kinds=ANY,
       needs=("complete rows",))


# -- prototypes ----------------------------------------------------------------------------------------------------------
def run_set_weights(be, st, args):
    be.set_weights(st.W)
    return (be.get_weights(0),)


op("set_weights", run_set_weights, ("dbgsom_ctx_set_weights", "dbgsom_ctx_get_weights"),
   after=after(bound=(CLEARS_SAME_BUFFER, cite("dbgsom_ctx_set_weights", "weights_replaced"))), kinds=ANY)


def _write_rows(st, args):
    how, r = args
    M, d = st.resident.shape
    rng = am.rng_for("write", st.cfg.name, how, r, M)
    return (M if how == "append" else r % M), st.W[:1] + 0.01 * rng.standard_normal((1, d))


def run_write_weight_rows(be, st, args):
    row0, rows = _write_rows(st, args)
    be.write_weight_rows(row0, rows)
    M = max(len(st.resident), row0 + 1)
    return (be.get_weights(0), be.read_weight_rows(np.array([row0, 0, M - 1])))


def ref_write_weight_rows(be, st, args):
    be.set_weights(st.resident)
    return run_write_weight_rows(be, st, args), {}


op("write_weight_rows", run_write_weight_rows, ("dbgsom_ctx_write_weight_rows", "dbgsom_ctx_get_weights", "dbgsom_ctx_read_weight_rows"),
   after=after(bound=(CLEARS_SAME_BUFFER, cite("dbgsom_ctx_write_weight_rows", "weights_replaced"))), ref=ref_write_weight_rows,
   kinds=("dense", "csr"),
   draw=lambda rng, st: (("append", "replace")[int(rng.integers(0, 2))], int(rng.integers(0, 1000))), needs=("resident prototypes",))
# (without resident prototypes row0 = M = 0 is an append on an empty map: the model keeps no map for that case, the
#  record is only drawn once prototypes are resident -- see `applies`)


def run_get_weights(be, st, args):
    return (be.get_weights(0),)


def ref_get_weights(be, st, args):
    be.set_weights(st.resident)
    return (be.get_weights(0),), {}


op("get_weights", run_get_weights, ("dbgsom_ctx_get_weights",), ref=ref_get_weights,
   refusal=lambda st, args: "holds 0 rows" if st.resident is None else None, kinds=ANY)


# -- the search of the resident rows and the reductions around it -----------------------------------------------------------
def run_bmu(k):
    def run(be, st, args):
        d, i = be.bmu(st.W, k)
        return (d, i)
    return run


_BMU = ("dbgsom_ctx_bmu", "dbgsom_ctx_bmu_masked")
op("bmu_k1", run_bmu(1), _BMU, after=AFTER_STAGED, kinds=ANY)
op("bmu_k2", run_bmu(2), _BMU, after=AFTER_STAGED, kinds=ANY)
op("resident_winners", lambda be, st, args: (be.resident_winners(st.W),), _BMU, after=AFTER_STAGED)
op("quantization_error", lambda be, st, args: (np.array([be.quantization_error(st.W)]),), ("dbgsom_ctx_quantization_error",),
   after=AFTER_STAGED)
op("topographic_error_count", lambda be, st, args: (np.array([be.topographic_error_count(st.W, coords_for(len(st.W)))],
                                                             dtype=np.float64),),
   ("dbgsom_ctx_topographic_count",), after=AFTER_STAGED)
op("node_statistics", lambda be, st, args: tuple(be.node_statistics(st.W, 2.0 * np.sqrt(st.cfg.d))), ("dbgsom_ctx_node_statistics",),
   after=AFTER_NODE_STATISTICS)


def r_labels(st, args=None):
    return "no labels attached" if st.labels is None else None


def _some_winners(st):
    return am.rng_for("winners", st.cfg.name, st.N, len(st.W)).integers(0, len(st.W), st.N)


_HIST = ("dbgsom_ctx_class_histogram",)


def run_class_histogram_weighted(be, st, args):
    """sample weights attached (they stay), then the histogram of summed weights"""
    if st.labels is not None:
        be.set_sample_weight(_weights(st))
    return (be.class_histogram(_some_winners(st), N_CLASSES, len(st.W)),)


op("class_histogram", lambda be, st, args: (be.class_histogram(_some_winners(st), N_CLASSES, len(st.W)),), _HIST,
   refusal=r_labels, needs=("labels",))


op("class_histogram_weighted", run_class_histogram_weighted, ("dbgsom_ctx_class_histogram_weighted", "dbgsom_ctx_set_sample_weight"),
   after=after(sums=(CLEARS, cite("dbgsom_ctx_set_sample_weight", "sumsM = 0"))), refusal=lambda st, args: r_labels(st),
   needs=("labels",))


def _read_M(st):
    return len(st.W) if st.winners is None else max(len(st.W), int(st.winners.max()) + 1)


def r_last_winners(first):
    def refusal(st, args=None):
        return first(st) or ("no winners of a previous epoch" if st.winners is None else None)
    return refusal


op("class_histogram_last", lambda be, st, args: (be.class_histogram(None, N_CLASSES, _read_M(st)),), _HIST,
   ref=lambda be, st, args: ((be.class_histogram(st.winners, N_CLASSES, _read_M(st)),), {}), refusal=r_last_winners(r_labels),
   needs=("labels", "the winners of an epoch"), reads=True, kinds=("dense", "csr"))


def r_targets(st, args=None):
    return "no targets attached" if st.targets is None else None


def _stats(t):
    return tuple(t)


op("target_statistics", lambda be, st, args: _stats(be.target_statistics(_some_winners(st), len(st.W), True, True)),
   ("dbgsom_ctx_target_statistics",), refusal=r_targets, needs=("targets",))
op("target_statistics_last", lambda be, st, args: _stats(be.target_statistics(None, _read_M(st), True, True)),
   ("dbgsom_ctx_target_statistics",), ref=lambda be, st, args: (_stats(be.target_statistics(st.winners, _read_M(st), True, True)), {}),
   refusal=r_last_winners(r_targets), needs=("targets", "the winners of an epoch"), reads=True, kinds=("dense", "csr"))


def run_unit_statistics(be, st, args):
    form = args
    rng = am.rng_for("unit", st.cfg.name, st.N)
    M = len(st.W)
    units, Y, w = rng.integers(0, M, st.N), rng.standard_normal((st.N, 3)), rng.random(st.N)
    if form == "device":
        Y = in_form(Y, "device", be)
    return tuple(host(a) for a in be.unit_statistics(units, Y, w, M, True, True))


op("unit_statistics", run_unit_statistics, ("dbgsom_ctx_unit_sums", "dbgsom_ctx_unit_sums_device", "dbgsom_ctx_unit_deviations_device"),
   draw=lambda rng, st: ("host", "device")[int(rng.integers(0, 2))])


def run_partition(be, st, args):
    counts, win = be.partition(st.W, True)
    return (counts, win)


def ref_partition(be, st, args):
    counts, win = be.partition(st.W, True)
    extras = {}
    if hasattr(be, "read_partition"):
        order, seg = be.read_partition()
        extras["part"] = (len(st.W), st.W, order, seg, counts)
    return (counts, win), extras


op("partition", run_partition, ("dbgsom_ctx_partition",), after=AFTER_PARTITION, ref=ref_partition, refusal=r_complete,
   needs=("complete rows",), kinds=ANY)
op("read_partition", lambda be, st, args: tuple(be.read_partition()), ("dbgsom_ctx_read_partition",),
   ref=lambda be, st, args: ((st.part[2], st.part[3]) if st.part is not None else tuple(be.read_partition()), {}),
   refusal=lambda st, args: "call dbgsom_ctx_partition first" if st.part is None else None, needs=("a partition",), reads=True,
   kinds=ANY)


def run_subset(be, st, args):
    unit = 0 if st.part is None else int(np.argmax(st.part[4]))
    sub = be.subset(unit)
    try:
        n = sub.n_samples
        return (np.array([n]), sub.read_samples(np.arange(n)))
    finally:
        sub.release()


def ref_subset(be, st, args):
    if st.part is not None:
        be.partition(st.part[1])
    return run_subset(be, st, args), {}


op("subset", run_subset, ("dbgsom_ctx_subset_create", "dbgsom_ctx_read_samples"), ref=ref_subset, kinds=("dense",),
   refusal=lambda st, args: "call dbgsom_ctx_partition first" if st.part is None else None, needs=("a partition",), reads=True)


def run_column_moments(be, st, args):
    m = be.column_moments()
    return () if m is None else (m[0], m[1], np.array([m[2]]))


op("column_moments", run_column_moments, ("dbgsom_ctx_column_sums",), refusal=r_complete, kinds=ANY)


def run_weighted_column_moments(be, st, args):
    total = be.weight_total()
    return (np.array([total]),) + tuple(be.weighted_column_moments(total))


op("weighted_column_moments", run_weighted_column_moments, ("dbgsom_ctx_weight_total", "dbgsom_ctx_weighted_column_sums"),
   refusal=lambda st, args: r_complete(st) or ("no weights attached" if st.sw is None else None)
   or ("the resident samples are CSR" if st.cfg.kind == "csr" else None), needs=("sample weights", "dense rows"))


def run_covariance_apply(be, st, args):
    rng = am.rng_for("cov", st.cfg.name)
    mean = np.nan_to_num(np.asarray(st.Xd, dtype=np.float64)).mean(axis=0)
    return tuple(be.covariance_apply(mean, rng.standard_normal((st.cfg.d, 3))))


op("covariance_apply", run_covariance_apply, ("dbgsom_ctx_covariance_apply",), refusal=r_metric,
   needs=("dense float32 / float64 rows", "complete rows", "no sample weights"), kinds=ANY)
op("read_sums", lambda be, st, args: (be.read_sums(len(st.W) if st.sums is None else st.sums[0]),), ("dbgsom_ctx_read_sums",),
   ref=lambda be, st, args: ((st.sums[1],) if st.sums is not None else (be.read_sums(len(st.W)),), {}), refusal=lambda st, args: "no sums of" if st.sums is None else None,
   needs=("the sums of an epoch",), reads=True, kinds=ANY)
op("read_samples", lambda be, st, args: (be.read_samples(np.array([0, st.N - 1, st.N // 2])),), ("dbgsom_ctx_read_samples",),
   kinds=("dense",))
op("exp_similarity", lambda be, st, args: (be.exp_similarity(np.linspace(0.0, 30.0, 777), st.gamma),), ("dbgsom_ctx_exp_similarity",))


# -- queries on other rows -----------------------------------------------------------------------------------------------
def draw_query(forms, with_k=False):
    def draw(rng, st):
        n, form = int(rng.choice(ROWS)), forms[int(rng.integers(0, len(forms)))]
        return (n, form, int(rng.choice(KS))) if with_k else (n, form)
    return draw


ALL_FORMS, DENSE_FORMS = ("host", "device", "csr"), ("host", "device")


def _q(be, st, args):
    return in_form(query_rows(st, args[0], args[1]), args[1], be)


def _variants(stem, forms):
    return tuple(stem + ("" if f == "host" else "_" + f) for f in forms)


def _holes(Q, key):
    Q = Q.copy()
    Q[am.rng_for("qholes", key, Q.shape).random(Q.shape) < 0.1] = np.nan
    return Q


for _metric, _forms in (("euclidean", ALL_FORMS), ("manhattan", DENSE_FORMS), ("cosine", DENSE_FORMS), ("masked", ("host",))):
    _sfx = "" if _metric == "euclidean" else "_" + _metric

    def _rows(be, st, args, masked=_metric == "masked"):
        Q = query_rows(st, args[0], args[1])
        return _holes(Q, st.cfg.name) if masked else in_form(Q, args[1], be)

    def _bmu_q(be, st, args, name="bmu" + _sfx, rows=_rows, eu=_metric == "euclidean"):
        k = min(args[2], 2)
        X = rows(be, st, args)
        return tuple(be.bmu(st.W, k, X)) if eu else tuple(getattr(be, name)(st.W, k, X))

    def _dist_q(be, st, args, name="distances" + _sfx, rows=_rows):
        return (getattr(be, name)(st.W, rows(be, st, args)),)

    def _kn_q(be, st, args, name="kneighbors" + _sfx, rows=_rows):
        return tuple(getattr(be, name)(st.W, args[2], rows(be, st, args)))

    _in = "" if _metric == "euclidean" else "_" + _metric
    _ent = (lambda stem, forms=_forms, infix=_in: tuple(f"dbgsom_ctx_{stem}{infix}" + ("" if f == "host" else "_" + f) for f in forms))
    op("query_bmu" + _sfx, _bmu_q, _ent("bmu_query"), draw=draw_query(_forms, True), kinds=ANY)
    op("query_distances" + _sfx, _dist_q, _ent("distances_query"), draw=draw_query(_forms, True), kinds=ANY)
    op("query_kneighbors" + _sfx, _kn_q, _ent("kneighbors_query"), draw=draw_query(_forms, True), kinds=ANY)


def run_bmu_metric(metric):
    def run(be, st, args):
        be.set_metric(metric)
        try:
            return tuple(be.bmu(st.W, args))
        finally:
            be.set_metric("euclidean")
    return run


for _m in ("manhattan", "cosine"):
    op("bmu_resident_" + _m, run_bmu_metric(_m), ("dbgsom_ctx_bmu_" + _m,), refusal=r_metric, kinds=ANY,
       draw=lambda rng, st: int(rng.integers(1, 3)), needs=("dense float32 / float64 rows", "complete rows", "no sample weights"))


def _H(M, sigma=1.5):
    return np.exp(-hop_for(M) ** 2 / (2.0 * sigma * sigma))


op("query_neighborhood_energy", lambda be, st, a: tuple(be.neighborhood_energy(st.W, _H(len(st.W)), _q(be, st, a))),
   _variants("dbgsom_ctx_distortion_query", ALL_FORMS), draw=draw_query(ALL_FORMS))
op("query_exemplars", lambda be, st, a: tuple(be.exemplars(st.W, a[2], _q(be, st, a), own_cell=a[0] > 1)),
   _variants("dbgsom_ctx_exemplars_query", ALL_FORMS), draw=draw_query(ALL_FORMS, True))
op("query_range_counts", lambda be, st, a: (be.range_counts(st.W, np.array([0.5, 1.5, 4.0]) * st.cfg.d, _q(be, st, a)),),
   _variants("dbgsom_ctx_range_counts_query", ALL_FORMS), draw=draw_query(ALL_FORMS))


def run_mixture(be, st, a):
    M = len(st.W)
    rng = am.rng_for("mixture", st.cfg.name, M)
    return tuple(be.mixture(st.W, np.log(rng.dirichlet(np.ones(M))), 0.5 / st.cfg.d, rng.standard_normal((M, 3)), _q(be, st, a)))


op("query_mixture", run_mixture, _variants("dbgsom_ctx_mixture_query", ALL_FORMS), draw=draw_query(ALL_FORMS))
op("query_combined_error", lambda be, st, a: tuple(be.combined_error(st.W, edges_for(len(st.W)), _q(be, st, a))),
   _variants("dbgsom_ctx_combined_error_query", ALL_FORMS), draw=draw_query(ALL_FORMS))
op("geodesics", lambda be, st, a: (be.geodesics(st.W, edges_for(len(st.W))),), ("dbgsom_ctx_geodesics",))


def r_row_neighbors(st, args=None):
    if st.cfg.kind == "csr":
        return "the resident samples are CSR"
    if _bf16(st):
        return "stored as bfloat16"
    if st.part is None:
        return "no valid partition"
    return "M is not the partition's" if st.part[0] != len(st.W) else None


def run_row_neighbors(be, st, a):
    return tuple(be.row_neighbors(st.W, a[2], min(a[2] + 1, 4), _q(be, st, a)))


def ref_row_neighbors(be, st, a):
    if st.part is not None:
        be.partition(st.part[1])
    return run_row_neighbors(be, st, a), {}


op("query_row_neighbors", run_row_neighbors, _variants("dbgsom_ctx_row_neighbors_query", DENSE_FORMS), ref=ref_row_neighbors,
   draw=draw_query(DENSE_FORMS, True), refusal=r_row_neighbors, kinds=("dense", "csr"), needs=("a partition on these prototypes",),
   reads=True)


def run_sparse_code(be, st, a):
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return (be.sparse_code(st.W, _q(be, st, a), max_iter=20),)


op("query_sparse_code", run_sparse_code, _variants("dbgsom_ctx_sparse_code", DENSE_FORMS),
   draw=lambda rng, st: ((1, 131)[int(rng.integers(0, 2))], DENSE_FORMS[int(rng.integers(0, 2))]))
op("query_topographic_function", lambda be, st, a: tuple(be.topographic_function(st.W, _q(be, st, a), coords_for(len(st.W)), True)),
   _variants("dbgsom_ctx_topographic_function", DENSE_FORMS), draw=draw_query(DENSE_FORMS))


# -- attachments and loads -------------------------------------------------------------------------------------------------
def _labels(st):
    return am.rng_for("labels", st.cfg.name, st.N).integers(0, N_CLASSES, st.N).astype(np.int32)


def _weights(st):
    w = am.rng_for("sw", st.cfg.name, st.N).random(st.N) + 0.25
    w[::17] = 0.0
    return w


def _targets(st):
    return am.rng_for("targets", st.cfg.name, st.N).standard_normal((st.N, N_TARGETS))


def run_attach(what):
    def run(be, st, args):
        value = {"labels": _labels, "sw": _weights, "targets": _targets}[what](st) if args.startswith("attach") else None
        if args == "attach_device":
            value = in_form(value, "device", be)
        {"labels": be.set_labels, "sw": be.set_sample_weight, "targets": be.set_targets}[what](value)
        return ()
    return run


_DRAW_ATTACH = (lambda rng, st: ("attach", "attach", "detach")[int(rng.integers(0, 3))])
op("set_labels", run_attach("labels"), ("dbgsom_ctx_set_labels",), draw=_DRAW_ATTACH, ref=lambda be, st, a: ((), {}), kinds=ANY)
op("set_sample_weight", run_attach("sw"), ("dbgsom_ctx_set_sample_weight",), draw=_DRAW_ATTACH, ref=lambda be, st, a: ((), {}),
   after=after(sums=(CLEARS_ON_ATTACH, cite("dbgsom_ctx_set_sample_weight", "sumsM = 0"))), kinds=("dense", "csr"))
op("set_targets", run_attach("targets"), ("dbgsom_ctx_set_targets", "dbgsom_ctx_set_targets_device"),
   draw=lambda rng, st: ("attach", "attach_device", "detach")[int(rng.integers(0, 3))],
   ref=lambda be, st, a: ((), {}), kinds=ANY)


def run_load(rows):
    def run(be, st, args):
        # "more": a load of N - 77 rows and then one of all N -- the resident row count grows behind a reload, and every
        # buffer sized by N is reserved again over what the smaller load left in it
        for n in {"same": (st.cfg.N,), "fewer": (st.cfg.N - 77,), "more": (st.cfg.N - 77, st.cfg.N)}[rows]:
            X = st.X if n == st.cfg.N else st.X[:n]
            if getattr(be, "name", "") == "hip":
                be.load(X, storage="bf16" if _bf16(st) else None, incomplete=st.cfg.kind == "incomplete")
            else:           # (the NumPy backends keep attachments across a load: detached here as the context does it)
                be.load(X)
                be.set_labels(None), be.set_sample_weight(None), be.set_targets(None)
        return (np.array([be.n_samples]),)
    return run


for _r in ("same", "fewer", "more"):
    op("load_" + _r, run_load(_r), ("dbgsom_ctx_load", "dbgsom_ctx_load_csr"), after=AFTER_LOAD, kinds=ANY,
       ref=lambda be, st, a, r=_r: ((np.array([{"same": st.cfg.N, "fewer": st.cfg.N - 77, "more": st.cfg.N}[r]]),), {}))

CLEARING = tuple(n for n, o in OPS.items() if any(v[0] not in (KEEPS, SETS) for v in o.after.values()))
READS = ("class_histogram_last", "target_statistics_last", "read_sums", "read_partition")
READ_FLAG = {"class_histogram_last": "last_idx_valid", "target_statistics_last": "last_idx_valid", "read_sums": "sums",
             "read_partition": "part_valid"}

# every dbgsom_ctx_* entry no record reaches, with the reason
EXCLUDED = {
    "dbgsom_ctx_create": "every context is made by it: the harness, not an operation between epochs",
    "dbgsom_ctx_destroy": "every release ends in it",
    "dbgsom_ctx_set_option": "the harness configures every context with it",
    "dbgsom_ctx_get_option": "the harness reads counters and flags with it; it changes nothing",
    "dbgsom_ctx_stream": "hands out the stream handle; no state",
    "dbgsom_ctx_load_device": "the load of rows in HBM ends in the same reset as dbgsom_ctx_load (tests/test_gpu_device_input.py)",
    "dbgsom_ctx_set_allreduce": "more than one rank: tests/test_gpu_distributed.py",
    "dbgsom_ctx_set_collectives": "called once by every HipBackend; more than one rank: tests/test_gpu_distributed.py",
    "dbgsom_ctx_set_rccl": "RCCL: more than one rank",
    "dbgsom_ctx_allreduce_host": "more than one rank",
    "dbgsom_ctx_scan_cells_device": "the raw scan of row_neighbors on caller-owned buffers: tests/test_gpu_row_neighbors.py",
    "dbgsom_ctx_arm_ms": "timing read-out",
    "dbgsom_ctx_phase_ms": "timing read-out",
    "dbgsom_ctx_filter_counts": "read-out of the last filtered search's list lengths: depends on the algorithm by design",
    "dbgsom_ctx_refine_counts": "read-out of the last filtered search's refinement counters",
    "dbgsom_ctx_read_anchors": "read-out of the anchor buckets: tests/test_gpu_anchor_seeds.py",
    "dbgsom_ctx_read_anchor_runs": "read-out of the anchor buckets' run table: tests/test_gpu_anchor_seeds.py",
}


# ----------------------------------------------------------------------------------------------------------------------
# running one step
# ----------------------------------------------------------------------------------------------------------------------
def applies(o, st):
    """whether a record is drawn in this state at all (what it needs beyond that is refused, not skipped)"""
    if st.cfg.kind not in o.kinds:
        return False
    if o.name == "write_weight_rows":
        return st.resident is not None
    return True


def draw_args(o, rng, st):
    return o.draw(rng, st) if o.draw else None


def hip_backend(cfg, algorithm=None):
    from dbgsom_amd.backend import HipBackend

    be = HipBackend(0, algorithm=algorithm or cfg.algorithm)
    be.sweep_planes = 4     # the pruning form: the arm that takes the hinted bound and the anchor seeds
    be.seed_stride = 4
    if cfg.refine is not None:
        be.refine = cfg.refine
    if cfg.kind == "csr":
        be.csr_densify_below = 0
    return be


def attach(be, st):
    """the resident rows and attachments of the model, on `be`"""
    if getattr(be, "name", "") == "hip":
        be.load(st.rows(), storage="bf16" if _bf16(st) else None, incomplete=st.cfg.kind == "incomplete")
    else:
        be.load(st.rows())
    if st.labels is not None:
        be.set_labels(st.labels)
    if st.sw is not None:
        be.set_sample_weight(st.sw)
    if st.targets is not None:
        be.set_targets(st.targets)
    return be


ERRORS = (RuntimeError, ValueError, IndexError, TypeError)
_REFERENCES = {}


def reference(o, st, args, factory):
    """what a fresh context returns for this one call -> (result, extras); results of equal calls in equal states are
    computed once"""
    key = (o.name, repr(args), st.digest(), None if st.winners is None else hashlib.blake2b(st.winners.tobytes(), digest_size=8).hexdigest(),
           None if st.part is None else st.part[0], None if st.sums is None else st.sums[0])
    if key not in _REFERENCES:
        be = attach(factory(st.cfg, "exact"), st)
        try:
            res = (o.ref or (lambda b, s, a: (o.run(b, s, a), {})))(be, st, args)
        finally:
            be.release()
        _REFERENCES[key] = (tuple(host(a) for a in res[0]), res[1])
        if len(_REFERENCES) > 4096:
            _REFERENCES.pop(next(iter(_REFERENCES)))
    return _REFERENCES[key]


def apply_effect(o, st, args, extras):
    """the model behind a call that went through"""
    name = o.name
    # a map with rows that are not finite goes to no later call: the walk ends here, by an assertion
    assert extras.get("W_out") is None or np.isfinite(extras["W_out"]).all(), \
        f"{name}: the new map has rows that are not finite -- the walk's inputs left the maps the calls are held to"
    if name == "epoch_masked":
        st.W = extras["W_out"]
    elif name in EPOCHS or name in GROWTHS or name in ("update", "epoch_manhattan", "epoch_cosine"):
        if not extras["frozen"]:
            st.W = st.resident = extras["W_out"]
        elif st.resident is None:
            st.resident = extras["W_in"]
    elif name in ("set_weights", "bmu_k1", "bmu_k2", "resident_winners", "quantization_error", "topographic_error_count",
                  "node_statistics", "partition") or (name == "set_hint_true" and (st.winners is None or st.winners.max() >= len(st.W))):
        if st.cfg.kind != "incomplete" or name == "set_weights":
            st.resident = st.W
    elif name == "write_weight_rows":
        row0, rows = _write_rows(st, args)
        W = st.resident if row0 < len(st.resident) else np.vstack([st.resident, rows])
        W = W.copy()
        W[row0] = rows[0]
        st.W = st.resident = np.ascontiguousarray(W)
    elif name.startswith("load_"):
        st.reload(st.cfg.N - 77 if name == "load_fewer" else st.cfg.N)
        return
    elif name == "class_histogram_weighted":
        st.sw = _weights(st)
    elif name == "set_labels":
        st.labels = _labels(st) if args == "attach" else None
    elif name == "set_sample_weight":
        st.sw = _weights(st) if args == "attach" else None
        if args == "attach":
            st.sums = None
    elif name == "set_targets":
        st.targets = _targets(st) if args.startswith("attach") else None
    for flag, attr, key in (("last_idx_valid", "winners", "winners"), ("part_valid", "part", "part"), ("sums", "sums", "sums")):
        verb = o.after[flag][0]
        if verb == SETS:
            setattr(st, attr, extras.get(key))
        elif verb == CLEARS:
            setattr(st, attr, None)


def step(be, st, o, args, factory):
    """One call on the context under test against the fresh context -> "ok" or "refused".  A refusal must be the one the
    record names, on both contexts, and leaves the model as it was."""
    refusal = o.expected_refusal(st, args)
    if refusal is not None:
        for who, ctx in (("the context under test", be), ("a fresh context", None)):
            try:
                if ctx is None:        # (a read is refused behind what the model says came before it, any other
                    fresh = attach(factory(st.cfg, "exact"), st)      # call as the first call of the context)
                    if st.resident is not None and hasattr(fresh, "set_weights"):
                        fresh.set_weights(st.resident)
                    try:
                        (o.ref if o.reads and o.ref else o.run)(fresh, st, args)
                    finally:
                        fresh.release()
                else:
                    o.run(ctx, st, args)
            except ERRORS as e:
                assert refusal in str(e) or not refusal, f"{o.name} on {who}: refused with {e!r}, expected '{refusal}'"
            else:
                raise AssertionError(f"{o.name} on {who}: expected the refusal '{refusal}', the call went through")
        return "refused"
    want, extras = reference(o, st, args, factory)
    got = o.run(be, st, args)
    assert_same(got, want, f"{o.name}{'' if args is None else repr(args)}")
    if (o.name in EPOCHS or o.name in GROWTHS) and oracle_applies(st):
        assert_oracle_epoch(st, extras["W_in"], got)
    apply_effect(o, st, args, extras)
    return "ok"


def probe_flags(be, st):
    """what the context itself says about its cached state, through calls that change none of it -> dict"""
    from dbgsom_amd._native import DbgsomNativeError

    def goes(fn):
        try:
            fn()
            return True
        except (DbgsomNativeError, ValueError):
            return False
    flags = {"hint_valid": bool(be._get("hint_valid")), "part_valid": goes(be.read_partition)}
    M = be._last_M or len(st.W)
    flags["sums"] = goes(lambda: be.read_sums(M))
    if st.labels is not None:
        flags["last_idx_valid"] = goes(lambda: be.class_histogram(None, N_CLASSES, 16000))
    return flags


def expected_flags(o, before, args=None):
    """what `probe_flags` must read behind the call (the bound has no probe: tests (b) of the GPU file count its uses)"""
    out = {}
    for flag, was in before.items():
        verb = o.after[flag][0]
        clears = verb == CLEARS or (verb == CLEARS_ON_ATTACH and args == "attach")
        out[flag] = True if verb == SETS else False if clears else was
    return out


# ----------------------------------------------------------------------------------------------------------------------
# seeded walks
# ----------------------------------------------------------------------------------------------------------------------
def walk(seed, cfg, steps=WALK_STEPS):
    """A list of (op name, args or None: drawn from the state when the step runs).  The walks of one configuration share
    one permutation of the records that apply to it, each seed taking every third, an epoch behind every second call and
    directly behind every call that clears a flag; then, for every read of what an epoch left, epoch -> a clearing call
    -> the read.  Cut to `steps` (padded with drawn calls when shorter): tests/test_call_order_cpu.py holds the cut
    walks against the coverage they owe."""
    rng = np.random.default_rng(zlib.crc32(repr(("walk", cfg.name)).encode()))
    names = [n for n, o in OPS.items() if cfg.kind in o.kinds and n not in EPOCHS]
    names = [names[i] for i in rng.permutation(len(names))]
    mine = names[seed % len(WALK_SEEDS)::len(WALK_SEEDS)]
    rng = np.random.default_rng(zlib.crc32(repr(("walk", cfg.name, seed)).encode()))
    forms = ("epoch_resident", "epoch", "epoch_frozen")
    seq = ["set_labels+", "set_targets+", "epoch_resident", "epoch_resident"]
    for i, n in enumerate(mine):
        seq.append(n)
        if n in CLEARING or i % 2:
            seq.append(forms[int(rng.integers(0, 3))])
    for i, read in enumerate(READS):
        if cfg.kind not in OPS[read].kinds:
            continue
        if cfg.kind == "incomplete":      # (no call sets what the reads read on rows with missing entries: all refused)
            seq.append(read)
            continue
        flag = READ_FLAG[read]
        setter = "partition" if flag == "part_valid" else "epoch_resident"
        # (not the metric epochs: refused on bfloat16 and CSR residents and with weights attached, they would clear nothing)
        mine = [n for n in CLEARING if cfg.kind in OPS[n].kinds and not n.startswith(("load_", "epoch_manhattan", "epoch_cosine"))]
        drops = [n for n in mine if OPS[n].after[flag][0] not in (KEEPS, SETS)]
        others = [n for n in mine if OPS[n].after[flag][0] == KEEPS and n not in EPOCHS + GROWTHS]
        # ... behind a call that clears something else (the read still answers), and behind one that clears what it reads
        drop = drops[(seed + i) % len(drops)]
        seq += [setter, others[(seed + i) % len(others)], read, setter, drop + "+" * (drop == "set_sample_weight"), read]
    while len(seq) < steps:
        seq.append(names[int(rng.integers(0, len(names)))])
    out = []
    for n in seq[:steps]:
        if n.endswith("+"):
            out.append((n[:-1], "attach"))
        else:                          # (no record's draw looks at the state: a walk is its names and arguments)
            out.append((n, draw_args(OPS[n], rng, None)))
    return out


def run_walk(be, st, steps, factory, seed=0, log=None):
    """-> the outcomes, one per step"""
    rng = np.random.default_rng(zlib.crc32(repr(("args", st.cfg.name, seed)).encode()))
    done = []
    for name, args in steps:
        o = OPS[name]
        if not applies(o, st):                 # (write_weight_rows without a resident map: set one first, then the call)
            step(be, st, OPS["set_weights"], None, factory)
        if args is None:
            args = draw_args(o, rng, st)
        done.append(step(be, st, o, args, factory))
        if log is not None:
            log(name, args, done[-1])
    return done
