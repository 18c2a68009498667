"""MI355X: any call between two epochs of a context leaves every later result what a fresh context computes.

tests/call_order.py holds the op table, the stateless reference (a fresh ``algorithm="exact"`` context per call, released
afterwards) and the walks; this file drives them on the device at the smallest shapes the filtered forms run at
(tests/test_gpu_lean_anchor_epoch.py's), with ``sweep_planes = 4`` / ``seed_stride = 4``: the pruning arm, the one that
takes the hinted bound (``hint_bound_searches``) and the anchor seeds.

  a. E, E, op, E, E -- resident evolving maps and frozen ones: every call the fresh context's, the flags behind `op` the
     table's, and (b) the hinted bound in use in front of `op` and not taken behind a call that drops it;
  c. the reads of what an epoch left, behind every call of the table: the epoch's answer or the state error;
  d. (the seeded walks are not run here: see the note at d below);
  e. every query on other rows back to back through the shared buffers, larger to smaller and back;
  f. two contexts on one thread."""
import ctypes
import time
import zlib

import numpy as np
import pytest

from tests import call_order as co

pytestmark = pytest.mark.gpu

MODES = ("resident", "frozen")
COUNTERS = ("hint_bound_searches", "anchor_searches", "lean_searches")
NEEDS_PARTITION = ("read_partition", "subset", "query_row_neighbors")


def _cases():
    out = []
    for cfg in co.CONFIGS:
        for name, o in co.OPS.items():
            if cfg.kind in o.kinds:
                out.append(pytest.param(name, cfg, id=f"{name}-{cfg.name}"))
    return out


def _start(cfg, mode, attach=("set_labels", "set_targets")):
    """a context and its model behind the attachments and E, E -> (be, st, the epoch's record)"""
    st = co.State(cfg)
    st.sigma = co.SIGMA_FROZEN if mode == "frozen" else co.SIGMA_EVOLVING
    be = co.attach(co.hip_backend(cfg), st)
    for name in attach:
        co.step(be, st, co.OPS[name], "attach", co.hip_backend)
    if mode == "frozen" and cfg.kind != "incomplete":
        co.step(be, st, co.OPS["set_weights"], None, co.hip_backend)
    E = co.OPS["epoch_frozen" if mode == "frozen" else "epoch_resident"]
    outcome = [co.step(be, st, E, None, co.hip_backend) for _ in range(2)]
    if cfg.kind == "dense":
        assert outcome == ["ok", "ok"]
        info = be.epoch_info()
        assert info[0] == 1, "the configuration does not reach the filtered search"
        if cfg.hinted:
            assert info[3] == 1 and be._get("hint_valid") == 1, "the configuration does not reach the hinted search"
    return be, st, E


def _bound_kept(o, outcome, mode, args):
    """whether the pruning bound survives the call (the table's `bound` entry, read for this mode)"""
    verb = o.after["bound"][0]
    if outcome == "refused" or verb in (co.KEEPS, co.SETS):
        return True
    # a call that overwrites the resident matrix: the bound's own behind a frozen epoch, the other one behind an
    # epoch that swapped the buffers
    return verb == co.CLEARS_SAME_BUFFER and mode == "resident"


# ---- a, b ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cfg", _cases())
def test_one_call_between_epochs(name, cfg):
    o = co.OPS[name]
    for mode in MODES:
        be, st, E = _start(cfg, mode)
        if cfg.hinted:
            # (b) the hinted bound was taken in front of the call: the second epoch's search
            assert be._get("hint_bound_searches") >= 1, "the hinted pruning bound was not in use before the call"
        alive = True       # the bound, as far as the calls in front of `op` go
        if name in NEEDS_PARTITION:
            alive = _bound_kept(co.OPS["partition"], co.step(be, st, co.OPS["partition"], None, co.hip_backend), mode, None)
        before = co.probe_flags(be, st)
        rng = np.random.default_rng(zlib.crc32(repr((name, cfg.name, mode)).encode()))
        args = co.draw_args(o, rng, st)
        searches = {k: be._get(k) for k in COUNTERS}
        outcome = co.step(be, st, o, args, co.hip_backend)
        if name in co.EPOCHS and cfg.hinted:
            # an epoch as the call in between: hinted, and with the bound unless it uploads its prototypes over the
            # matrix the bound refers to (host W behind a frozen epoch: stage_weights -> weights_replaced)
            assert outcome == "ok" and be.epoch_info()[3] == 1
            own = be._get("hint_bound_searches") - searches["hint_bound_searches"]
            assert own == int(not (name == "epoch" and mode == "frozen")), f"{mode}: {name} took the bound {own} times"
        flags = co.probe_flags(be, st)
        want = before if outcome == "refused" else co.expected_flags(o, before, args)
        if name.startswith("load_") or (name == "set_labels" and args == "detach"):
            flags.pop("last_idx_valid", None), want.pop("last_idx_valid", None)     # (no labels: the probe has no say)
        for f in flags:
            if f in want:
                assert flags[f] == want[f], f"{mode}: {f} reads {flags[f]} behind {name}, the table says '{o.after[f][0]}'"
        taken = be._get("hint_bound_searches")
        after = co.step(be, st, E, None, co.hip_backend)
        if cfg.kind == "dense":
            assert after == "ok"
            hinted = bool(be.epoch_info()[3])
            bound = be._get("hint_bound_searches") - taken
            seeded = {k: be._get(k) - v for k, v in searches.items()}
            print(f"{cfg.name} {mode} {name}{'' if args is None else args}: {outcome}; the epoch behind it: "
                  f"{'hinted' if hinted else 'not hinted'}, bound {'taken' if bound else 'not taken'}; since the call: "
                  f"{seeded['anchor_searches']} anchor-seeded, {seeded['lean_searches']} lean")
            if cfg.hinted:
                assert hinted == flags["hint_valid"], "the hint's flag and the epoch's seeds disagree"
                assert bound == int(hinted and alive and _bound_kept(o, outcome, mode, args)), \
                    f"{mode}: the bound behind {name} ('{o.after['bound'][0]}'): taken {bound} times"
            else:
                assert not hinted and bound == 0
        co.step(be, st, E, None, co.hip_backend)
        be.release()


def test_the_bound_is_dropped_by_what_must_drop_it():
    """(b) by name: update, the metric epochs, set_hint, and set_weights / write_weight_rows on the bound's own matrix"""
    cfg = co.CONFIG["f32-hint"]
    for name, mode, kept in (("get_weights", "resident", True), ("get_weights", "frozen", True), ("update", "resident", False),
                             ("epoch_manhattan", "resident", False), ("epoch_cosine", "resident", False),
                             ("set_hint_true", "resident", False), ("set_hint_random", "frozen", False),
                             ("set_weights", "frozen", False), ("write_weight_rows", "frozen", False),
                             ("set_weights", "resident", True)):
        be, st, E = _start(cfg, mode, attach=())
        assert be._get("hint_bound_searches") == 1, "E, E: the second epoch takes the bound"
        args = ("replace", 7) if name == "write_weight_rows" else None
        assert co.step(be, st, co.OPS[name], args, co.hip_backend) == "ok"
        hinted_flag = be._get("hint_valid")
        co.step(be, st, E, None, co.hip_backend)
        assert be._get("hint_bound_searches") == 1 + int(kept and hinted_flag), (name, mode)
        be.release()


# ---- c ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [co.CONFIG[n] for n in ("f32-hint", "bf16-lean", "csr")], ids=lambda c: c.name)
def test_reads_behind_an_intervening_call(cfg):
    """E, partition, op, then class_histogram(None), target_statistics(None), read_sums(M), read_partition(): what the
    model holds -- the answer of the epoch's winners passed explicitly, the epoch's sums, the partition's order, all from
    fresh contexts -- or, where the call dropped what the read reads, the state error.  Nothing else."""
    answered = refused = 0
    for name, o in co.OPS.items():
        if cfg.kind not in o.kinds:
            continue
        st = co.State(cfg)
        be = co.attach(co.hip_backend(cfg), st)
        for first, a in (("set_labels", "attach"), ("set_targets", "attach"), ("epoch_resident", None), ("partition", None)):
            assert co.step(be, st, co.OPS[first], a, co.hip_backend) == "ok"
        rng = np.random.default_rng(zlib.crc32(repr(("reads", name, cfg.name)).encode()))
        co.step(be, st, o, co.draw_args(o, rng, st), co.hip_backend)
        for read in co.READS:
            outcome = co.step(be, st, co.OPS[read], None, co.hip_backend)
            answered, refused = answered + (outcome == "ok"), refused + (outcome == "refused")
        be.release()
    print(f"{cfg.name}: {answered} reads answered, {refused} refused")
    assert answered and refused


# ---- d ------------------------------------------------------------------------------------------------------------------
# The seeded walks of tests/call_order.py (`walk`, `run_walk`) are NOT run on the device.  A walk whose maps had turned into
# NaN rows (a narrow neighbourhood on a map that grew by a row: 0 / 0 for every unit without an active unit in reach;
# up to 234 of 255 rows) stopped making progress on the device and was ended by its time limit; which call of the
# context does not come back on such a map is not known.  Until it is, the walks stay a host-side
# generator with its coverage checks (tests/test_call_order_cpu.py) and nothing here runs them.


# ---- e ------------------------------------------------------------------------------------------------------------------
def test_queries_of_every_kind_back_to_back():
    """One context, no epoch in between: rows 700 -> 1 -> 131 on a map of 256 and then of 130 units hand kn_ws / kn_idx /
    kn_dist, pd_out, qidx / qdist, stage_dev and xq from a larger user to a smaller one and back."""
    cfg = co.CONFIG["f64-hint"]
    st = co.State(cfg)
    be = co.attach(co.hip_backend(cfg), st)
    W256 = st.W
    queries = [n for n in co.OPS if n.startswith("query_")] + ["geodesics"]
    compared = 0
    assert co.step(be, st, co.OPS["partition"], None, co.hip_backend) == "ok"
    for M in (256, 130):
        st.W = np.ascontiguousarray(W256[:M])
        for j, rows in enumerate((700, 1, 131)):
            order = queries if j % 2 == 0 else queries[::-1]
            for i, name in enumerate(order):
                o = co.OPS[name]
                forms = co.ALL_FORMS if "csr" in "".join(o.entries) else co.DENSE_FORMS if "_device" in "".join(o.entries) else ("host",)
                form = forms[(i + j) % len(forms)]
                args = None if o.draw is None else (min(rows, 131), form) if name == "query_sparse_code" else (rows, form, co.KS[(i + j) % 3])
                outcome = co.step(be, st, o, args, co.hip_backend)
                # (row_neighbors on 130 units: the partition is one of 256, the refusal is the expected outcome)
                assert outcome == ("refused" if name == "query_row_neighbors" and M == 130 else "ok"), (name, M, rows)
                compared += 1
    be.release()
    assert compared == 6 * len(queries)


# ---- f ------------------------------------------------------------------------------------------------------------------
def _script(cfg):
    """epochs and queries of one context: (op name, args)"""
    return [("epoch_resident", None), ("query_kneighbors", (131, "host", 5)), ("epoch_resident", None), ("query_mixture", (700, "host")),
            ("epoch_resident", None), ("bmu_k1", None), ("query_exemplars", (131, "device", 2)), ("epoch_resident", None),
            ("node_statistics", None), ("epoch_resident", None), ("query_combined_error", (1, "csr")), ("epoch_frozen", None)]


def _phase_ms(be):
    from dbgsom_amd import _native

    ms = (ctypes.c_double * 8)()
    _native.call("dbgsom_ctx_phase_ms", be._ctx, ms)
    return [float(v) for v in ms]


def test_two_contexts_on_one_thread():
    """A (4096 x 48, M = 130) and B (1000 x 70, M = 256) alternate epochs and queries: each one's outputs are its solo
    run's bit for bit, and with `timing` on A only B has no timings and A's are those of A's last epoch."""
    from dbgsom_amd._native import DbgsomNativeError

    cfgs = {"A": co.CONFIG["f32-hint"], "B": co.CONFIG["f64-hint"]}
    solo = {}
    for who, cfg in cfgs.items():
        st = co.State(cfg)
        be = co.attach(co.hip_backend(cfg), st)
        solo[who] = []
        for name, args in _script(cfg):
            solo[who].append(tuple(co.host(a) for a in co.OPS[name].run(be, st, args)))
            co.apply_effect(co.OPS[name], st, args, _extras(name, st, solo[who][-1]))
        be.release()
    sts = {who: co.State(cfg) for who, cfg in cfgs.items()}
    bes = {who: co.attach(co.hip_backend(cfg), sts[who]) for who, cfg in cfgs.items()}
    bes["A"]._set("timing", 1)
    a_ms = None
    for i, (name, args) in enumerate(_script(None)):
        for who in ("A", "B") if i % 2 == 0 else ("B", "A"):
            be, st = bes[who], sts[who]
            got = tuple(co.host(a) for a in co.OPS[name].run(be, st, args))
            co.assert_same(got, solo[who][i], f"context {who}, step {i} ({name})")
            co.apply_effect(co.OPS[name], st, args, _extras(name, st, got))
            if name in co.EPOCHS:
                if who == "A":
                    a_ms = _phase_ms(be)
                    assert all(v >= 0.0 for v in a_ms) and sum(a_ms[:3]) > 0.0
                else:
                    with pytest.raises(DbgsomNativeError, match="no timed epoch"):
                        _phase_ms(be)
                    if a_ms is not None:
                        assert _phase_ms(bes["A"]) == a_ms, "A's timings changed with a call on B"
    for be in bes.values():
        be.release()


def _extras(name, st, out):
    """the model's input behind a call of the solo / alternating runs (their own outputs: the comparison is between the
    two runs, the fresh-context reference is tests (a) to (e)'s)"""
    if name in co.EPOCHS:
        return {"winners": out[0], "W_in": st.W if st.resident is None else st.resident, "W_out": out[2], "frozen": name == "epoch_frozen",
                "sums": None}
    return {}
