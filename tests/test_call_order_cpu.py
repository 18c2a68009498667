"""CPU: the op table, the walks and the harness of tests/call_order.py.

The table must place every ``dbgsom_ctx_*`` entry of the ABI, its `after` column must be what ResidentSearchState
(csrc/epoch_control.h) itself does -- tests/call_order_flags.cpp, compiled with the host C++ compiler, prints the flags
behind every transition the column cites -- every citation must resolve to a line of the engine, the walks the GPU file
runs must owe no coverage, and the reference runner and the comparison helpers must catch what they are there to catch
(run here on the NumPy oracle backend)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from dbgsom_amd import _native
from tests import call_order as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dbgsom_amd", "csrc")


# ---- 1. the ABI -------------------------------------------------------------------------------------------------------
def test_every_context_entry_is_placed():
    ctx = {name for name in _native.SIGNATURES if name.startswith("dbgsom_ctx_")}
    reached = {e for o in co.OPS.values() for e in o.entries}
    assert not (reached | set(co.EXCLUDED)) - ctx, "names that are no entries of the ABI"
    assert not reached & set(co.EXCLUDED), "entries both reached and excluded"
    missing = sorted(ctx - reached - set(co.EXCLUDED))
    assert not missing, f"context entries neither reached by a record of the op table nor excluded with a reason: {missing}"
    assert all(isinstance(r, str) and len(r) > 10 for r in co.EXCLUDED.values())


def test_the_table_holds_what_the_issue_names():
    for name in ("epoch", "epoch_resident", "epoch_frozen", "update", "set_hint_true", "set_hint_random", "set_weights",
                 "write_weight_rows", "get_weights", "bmu_k1", "bmu_k2", "resident_winners", "quantization_error",
                 "topographic_error_count", "node_statistics", "class_histogram", "class_histogram_last", "target_statistics",
                 "target_statistics_last", "unit_statistics", "partition", "read_partition", "column_moments", "covariance_apply",
                 "read_sums", "query_bmu", "query_distances", "query_kneighbors", "query_neighborhood_energy", "query_exemplars",
                 "query_range_counts", "query_mixture", "query_combined_error", "query_row_neighbors", "query_sparse_code",
                 "query_topographic_function", "query_bmu_masked", "query_bmu_manhattan", "epoch_manhattan", "query_bmu_cosine",
                 "epoch_cosine", "set_labels", "set_sample_weight", "set_targets", "load_same", "load_fewer", "load_more", "growth",
                 "shrink", "duplicate", "class_histogram_weighted"):
        assert name in co.OPS, name
    for o in co.OPS.values():
        assert set(o.after) == set(co.FLAGS), o.name
        assert set(o.kinds) <= {"dense", "csr", "incomplete"} and o.kinds, o.name


# ---- 2. the walks -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", co.CONFIGS, ids=[c.name for c in co.CONFIGS])
def test_the_walks_owe_no_coverage(cfg):
    walks = [[n for n, _ in co.walk(seed, cfg)] for seed in co.WALK_SEEDS]
    assert all(len(w) == co.WALK_STEPS for w in walks)
    assert walks == [[n for n, _ in co.walk(seed, cfg)] for seed in co.WALK_SEEDS], "a walk is not a function of its seed"
    seen = set().union(*walks)
    owed = sorted(n for n, o in co.OPS.items() if cfg.kind in o.kinds and n not in seen)
    assert not owed, f"records that apply to {cfg.name} and stand in none of its walks: {owed}"
    # every call that clears a flag is followed by an epoch at least once
    for name in co.CLEARING:
        if cfg.kind not in co.OPS[name].kinds or name in co.EPOCHS:
            continue
        assert any(w[i] == name and w[i + 1] in co.EPOCHS for w in walks for i in range(len(w) - 1)), name
    # every read of what an epoch (or a partition) left stands at least once behind setter -> a clearing call -> read,
    # with a call that clears what it reads and with one that clears something else
    for read in co.READS:
        if cfg.kind not in co.OPS[read].kinds or cfg.kind == "incomplete":    # (incomplete rows: every read is refused)
            continue
        flag = co.READ_FLAG[read]
        found = set()
        for w in walks:
            for i, n in enumerate(w):
                if n != read:
                    continue
                back = w[:i][::-1]
                setter = next((j for j, m in enumerate(back) if co.OPS[m].after[flag][0] == co.SETS), None)
                for m in back[:setter or 0]:
                    if m in co.CLEARING:
                        found.add(co.OPS[m].after[flag][0] == co.KEEPS)
        assert found == {True, False}, f"{read}: the walks of {cfg.name} lack a clearing call between the epoch and the read"


@pytest.mark.parametrize("cfg", co.DENSE, ids=[c.name for c in co.DENSE])
def test_the_walks_spread_their_arguments(cfg):
    """a walk is its names AND arguments: over the walks of a configuration every row count, every k and every form of
    the rows occurs, rows grow behind a reload, and targets go up from the host and from the device"""
    steps = [s for seed in co.WALK_SEEDS for s in co.walk(seed, cfg)]
    assert steps == [s for seed in co.WALK_SEEDS for s in co.walk(seed, cfg)]
    queries = [a for n, a in steps if n.startswith("query_") and a is not None]
    assert {a[0] for a in queries} == set(co.ROWS)
    assert {a[1] for a in queries} == set(co.ALL_FORMS)
    assert {a[2] for a in queries if len(a) > 2} == set(co.KS)
    assert any(n == "load_more" for n, _ in steps) and any(n == "load_fewer" for n, _ in steps)
    assert all(a is not None for n, a in steps if co.OPS[n].draw is not None)


def test_drawn_arguments_stay_in_their_sets():
    st = co.State(co.Config("tiny", 300, 7, 20, "float64", "exact"))
    rng = np.random.default_rng(0)
    rows, ks, growth = set(), set(), set()
    for _ in range(200):
        n, form, k = co.OPS["query_kneighbors"].draw(rng, st)
        rows.add(n), ks.add(k)
        assert form in co.ALL_FORMS
        growth.add(co.OPS["growth"].draw(rng, st))
    assert rows == set(co.ROWS) == {1, 131, 700} and ks == set(co.KS) == {1, 2, 5} and growth == set(co.GROWTH) == {1, 3}


# ---- 3. the `after` column against the header ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flags():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler (c++ / g++) on PATH"
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "call_order_flags")
        subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "call_order_flags.cpp")], check=True)
        names = ["dense_search_done", "foreign_search_begun", "foreign_search_done", "caller_winners_taken", "sums_made",
                 "epoch_failed", "hint_seeded", "weights_replaced_bound", "weights_replaced_other", "bucket_order_rewritten", "reset"]
        out = subprocess.run([exe], input="".join(n + "\n" for n in names), capture_output=True, text=True, check=True)
    table = {}
    for ln in out.stdout.splitlines():
        name, *bits = ln.split()
        b = [int(v) for v in bits]
        table[name] = {f: {(0, 1): co.KEEPS, (1, 1): co.SETS, (0, 0): co.CLEARS}[(b[i], b[i + 3])]
                       for i, f in enumerate(("hint_valid", "last_idx_valid", "bound"))}
    print(table)
    assert set(table) == set(names)
    return table


STATE_FLAGS = ("hint_valid", "last_idx_valid", "bound")


def _transition(token):
    return "reset" if token == "search.reset" else token


def test_cited_transitions_do_what_the_table_says(flags):
    checked = 0
    for o in co.OPS.values():
        for f in STATE_FLAGS:
            verb, where = o.after[f]
            if where is None:
                continue
            token = _transition(where[2])
            if token == "weights_replaced":
                assert f == "bound" and verb == co.CLEARS_SAME_BUFFER, (o.name, f)
                assert flags["weights_replaced_bound"]["bound"] == co.CLEARS and flags["weights_replaced_other"]["bound"] == co.KEEPS
                for g in ("hint_valid", "last_idx_valid"):
                    assert flags["weights_replaced_bound"][g] == co.KEEPS
            else:
                assert token in flags, (o.name, f, token)
                assert flags[token][f] == verb, f"{o.name}: {f} is '{verb}' in the table, {token} '{flags[token][f]}' in the header"
            checked += 1
    assert checked >= 30


def test_calls_that_are_one_transition_match_it_flag_for_flag(flags):
    for name, token in co.ONE_TRANSITION.items():
        o = co.OPS[name]
        for f in STATE_FLAGS:
            verb = o.after[f][0]
            if verb == co.CLEARS_SAME_BUFFER:
                verb = co.CLEARS
            assert flags[token][f] == verb, f"{name}: {f} is '{verb}' in the table, '{flags[token][f]}' behind {token}"


def _function_body(text, function):
    """-> (first line number, lines) of the definition of `function` in a source text"""
    lines = text.splitlines()
    for i, ln in enumerate(lines):
        if re.match(r"^(static\s+)?[\w:<>\*&\s]+\b%s\(" % re.escape(function), ln) and not ln.startswith((" ", "\t", "//")) \
                and not ln.rstrip().endswith(";"):
            for j in range(i, len(lines)):
                if lines[j].startswith("}"):
                    return i + 1, lines[i:j + 1]
    raise AssertionError(f"no definition of {function}")


def test_every_citation_resolves_to_a_line():
    texts = {}
    cited = {}
    for o in co.OPS.values():
        for f, (verb, where) in o.after.items():
            assert (where is None) == (verb == co.KEEPS), (o.name, f)
            if where is None:
                continue
            file, function, token = where
            text = texts.setdefault(file, open(os.path.join(CSRC, file)).read())
            first, body = _function_body(text, function)
            hits = [first + k for k, ln in enumerate(body) if token in ln]
            assert hits, f"{o.name}: {f} cites '{token}' in {function} of {file}, which does not name it"
            cited[(file, function, token)] = hits[0]
    for (file, function, token), line in sorted(cited.items(), key=lambda kv: kv[1]):
        print(f"csrc/{file}:{line}: {function}: {token}")


# ---- 4. the harness on the NumPy oracle backend --------------------------------------------------------------------------
TINY = co.Config("tiny", 300, 7, 20, "float64", "exact")


def _oracle(cfg, algorithm=None):
    from oracle.som_oracle import OracleBackend

    return OracleBackend()


ORACLE_STEPS = [("set_labels", "attach"), ("set_targets", "attach"), ("epoch", None), ("bmu_k1", None), ("bmu_k2", None),
                ("quantization_error", None), ("topographic_error_count", None), ("node_statistics", None), ("class_histogram", None),
                ("target_statistics", None), ("growth", 1), ("epoch", None), ("update", None), ("duplicate", "duplicate"),
                ("shrink", "shrink"), ("partition", None), ("load_same", None), ("target_statistics", None), ("epoch", None)]


def test_a_walk_on_the_oracle_backend():
    st = co.State(TINY)
    st.sigma = co.SIGMA_WALK
    be = co.attach(_oracle(TINY), st)
    log = []
    done = co.run_walk(be, st, ORACLE_STEPS, _oracle, log=lambda *a: log.append(a))
    assert len(done) == len(ORACLE_STEPS) == len(log)
    # target_statistics behind the load: the targets went with the rows, the call is refused and nothing else changed
    assert done[-2] == "refused" and done.count("refused") == 1
    assert st.W.shape == (TINY.M, TINY.d)       # (one row grown, one dropped)
    assert st.labels is None and st.targets is None


class _OffByOne:
    """an oracle backend whose k = 1 search reports one winner wrongly: what the harness must catch"""

    def __init__(self, inner):
        self._inner = inner

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def bmu(self, W, k=1, X=None):
        d, i = self._inner.bmu(W, k, X)
        i = i.copy()
        i.reshape(-1)[17] ^= 1
        return d, i


def test_the_harness_catches_a_wrong_winner_and_a_missing_refusal():
    st = co.State(TINY, key="wrong")
    be = _OffByOne(co.attach(_oracle(TINY), st))
    with pytest.raises(AssertionError, match="bmu_k1: result 1 is not the fresh context's"):
        co.step(be, st, co.OPS["bmu_k1"], None, _oracle)
    # a call that must be refused and goes through
    st.targets = None
    be._inner.set_targets(np.zeros((TINY.N, 2)))
    with pytest.raises(AssertionError, match="expected the refusal 'no targets attached'"):
        co.step(be, st, co.OPS["target_statistics"], None, _oracle)


def test_comparison_is_bit_for_bit_with_every_nan_as_one():
    a = np.array([0.0, 1.0, np.nan])
    b = a.copy()
    b.view(np.uint64)[2] ^= np.uint64(1)                       # another NaN payload
    assert np.isnan(b[2]) and co.same((a,), (b,)) is None
    assert co.same((a,), (np.array([-0.0, 1.0, np.nan]),)) == 0             # -0.0 is not 0.0
    assert co.same((a,), (np.nextafter(a, 2.0),)) == 0
    assert co.same((a, None), (a, None)) is None and co.same((a, None), (a, a)) == 1
    assert co.same((np.arange(3),), (np.arange(3.0),)) == 0                  # integers are no floats
    assert co.same((a,), (a, a)) == -1
    assert co.same((a.reshape(3, 1),), (a,)) == 0


def test_expected_flags_follow_the_table():
    before = {"hint_valid": True, "last_idx_valid": True, "part_valid": True, "sums": True}
    assert co.expected_flags(co.OPS["node_statistics"], before) == {"hint_valid": False, "last_idx_valid": True, "part_valid": False,
                                                                  "sums": False}
    assert co.expected_flags(co.OPS["set_hint_random"], before) == {"hint_valid": True, "last_idx_valid": False, "part_valid": False,
                                                                  "sums": True}
    assert co.expected_flags(co.OPS["set_sample_weight"], before, "detach") == before
    assert co.expected_flags(co.OPS["set_sample_weight"], before, "attach") == dict(before, sums=False)
    none = dict.fromkeys(before, False)
    assert co.expected_flags(co.OPS["epoch_resident"], none) == {"hint_valid": True, "last_idx_valid": True, "part_valid": False,
                                                                "sums": True}
    assert co.expected_flags(co.OPS["query_mixture"], before) == before and co.expected_flags(co.OPS["load_fewer"], before) == none


def test_bf16_rounding_is_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -7, -3.1415927], dtype=np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.140625], dtype=np.float32)
    assert np.array_equal(co.bf16_round(x), want)
