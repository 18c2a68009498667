"""The policy of the filtered search (dbgsom_amd/csrc/search_policy.h) on the CPU: tests/policy_replay.cpp is
compiled with the host C++ compiler and fed traces of policy calls.

* The traces under tests/data/policy_traces/ were recorded from the policy as it stood inside engine.hip before it
  moved into the header (NAME.trace: the calls, NAME.expect: what that code answered); the header must answer the same,
  character for character (doubles are printed with %a).
* The scenario tests restate, without a GPU, what tests/test_gpu_parity.py asserts about the policy on 160 000-row inputs.
* The constants dbgsom_amd/backend.py mirrors by hand are compared with the header's.

To look at a decision: build the driver (see `driver` below), write the calls one per line (the format is at the top
of policy_replay.cpp) and pipe them in.
"""
import glob
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACES = os.path.join(ROOT, "tests", "data", "policy_traces")
AUTO, EXACT, FILTERED, FILTERED_HINT = 0, 1, 2, 3


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler (c++ / g++) on PATH"
    exe = str(tmp_path_factory.mktemp("policy") / "policy_replay")
    # plain host C++: nothing of ROCm on the include path
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "dbgsom_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "policy_replay.cpp")], check=True)
    return exe


def test_header_is_host_only():
    text = open(os.path.join(ROOT, "dbgsom_amd", "csrc", "search_policy.h")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes == ["<math.h>", "<stdint.h>", '"../../include/dbgsom_hip.h"']
    for word in ("hipStream_t", "hipError_t", "DevBuf", "dbgsom_ctx *", "hip_runtime", "__global__", "chrono"):
        assert word not in text, word


# ------------------------------------------------------------------------------------------------------------------
# recorded traces
# ------------------------------------------------------------------------------------------------------------------
TRACE_NAMES = sorted(os.path.basename(p)[:-6] for p in glob.glob(os.path.join(TRACES, "*.trace")))


def test_traces_are_there():
    assert len(TRACE_NAMES) >= 20
    assert sum(os.path.getsize(p) for p in glob.glob(os.path.join(TRACES, "*"))) < 256 * 1024


@pytest.mark.parametrize("name", TRACE_NAMES)
def test_trace_replays_to_the_recorded_output(driver, name):
    with open(os.path.join(TRACES, name + ".trace")) as f:
        got = subprocess.run([driver], stdin=f, capture_output=True, text=True, check=True).stdout
    want = open(os.path.join(TRACES, name + ".expect")).read()
    got_lines, want_lines = got.splitlines(), want.splitlines()
    for i, (g, w) in enumerate(zip(got_lines, want_lines)):
        assert g == w, f"{name}: output line {i + 1}"
    assert len(got_lines) == len(want_lines)
    assert got == want


# ------------------------------------------------------------------------------------------------------------------
# scenarios
# ------------------------------------------------------------------------------------------------------------------
class Policy:
    """One policy behind the driver, step by step."""

    def __init__(self, exe, algorithm, M=1024, N=160000, dp=784, **options):
        self.p = subprocess.Popen([exe], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1)
        self._send(f"opt algorithm {algorithm}")
        for k, v in options.items():
            self._send(f"opt {k} {v}")
        self.shape(M, N, dp)

    def _send(self, line, reply=False):
        self.p.stdin.write(line + "\n")
        self.p.stdin.flush()
        return self.p.stdout.readline().split() if reply else None

    def close(self):
        self.p.stdin.close()
        assert self.p.wait() == 0

    def shape(self, M, N, dp):
        self.M, self.N, self.dp, self.nb = M, N, dp, (N + 127) // 128
        self._send(f"shape {M} {N} {dp}")

    def allowed(self):
        return self._send("allowed", True)[1] == "1"

    def plan(self, hinted=False, training=True, bound=False):
        r = self._send(f"plan {int(hinted)} {int(training)} {int(bound)}", True)
        assert r[0] == "p"
        keys = ("planes", "seed_full", "probe", "retry", "hint_bound", "seed_stride", "sweep_planes", "refine",
                "refine_rows", "timing_form")
        out = dict(zip(keys, map(int, r[1:11])))
        out["guard_mean"] = float.fromhex(r[11])
        return out

    @staticmethod
    def _state(r):
        assert r[0] == "s"
        keys = ("planes_used", "planes_next", "seed_mode", "prune_retry", "plane_hold", "filter_backoff", "probe_next",
                "hinted", "seed_full", "probed")
        out = dict(zip(keys, map(int, r[1:11])))
        out["last_mean"], out["probe_mean"], out["arm_ms"] = (float.fromhex(x) if x not in ("nan", "-nan") else math.nan
                                                              for x in r[11:14])
        return out

    def observe(self, lists, probe_lists=0.0, retry_groups=0, frozen=True, ms=math.nan):
        ms = "nan" if math.isnan(ms) else repr(float(ms))
        return self._state(self._send(f"observe {round(lists * self.nb)} {round(probe_lists * self.nb)} {retry_groups} "
                                      f"{int(frozen)} {ms}", True))

    def exact_epoch(self):
        return self._state(self._send("exact_epoch", True))

    def guarded(self):
        self._send("guarded")

    def refine_timed(self, form, ms):
        self._send(f"refine_timed {form} {ms!r}")

    def k2(self, hinted=False):
        r = self._send(f"k2 {int(hinted)}", True)
        return r[1] == "1"

    def cost(self, seeds, planes, lists):
        return float.fromhex(self._send(f"cost {seeds} {planes} {lists!r}", True)[1])


def run_epochs(pol, n, lists, ms=None, hinted_after_first=False, retry_groups=None, frozen=True):
    """n training epochs of a world `lists(row, planes, retry) -> mean list length`; returns [(plan, state)].
    An epoch is timed (ms(row, planes)) when nothing rides along, as in the engine."""
    log = []
    for e in range(n):
        hinted = hinted_after_first and e > 0
        if not pol.allowed():
            log.append((None, pol.exact_epoch()))
            continue
        pl = pol.plan(hinted=hinted, bound=e > 0)
        row = 2 if hinted else pl["seed_full"]
        mean = lists(row, pl["planes"], pl["retry"])
        is_guarded = pl["guard_mean"] > 0 and mean > pl["guard_mean"]
        if is_guarded:
            pol.guarded()
        if pl["timing_form"] >= 0 and not is_guarded:
            pol.refine_timed(pl["timing_form"], ms(row, pl["planes"]) if ms else 5.0)
        clean = ms is not None and not pl["probe"] and not is_guarded and pl["timing_form"] < 0
        groups = retry_groups(row, pl["planes"], pl["retry"]) if retry_groups and (pl["planes"] == 0 or pl["probe"]) else 0
        st = pol.observe(mean, lists(row, 0, pl["retry"]) if pl["probe"] else 0.0, groups, frozen,
                         ms(row, pl["planes"]) if clean else math.nan)
        log.append((pl, st))
    return log


def test_backoff_doubles_to_its_cap_and_waits_for_unexplored_arms(driver):
    """tests/test_gpu_parity.py test_auto_policy_backs_off_on_near_duplicate_prototypes: every arm leaves 0.9 M."""
    M = 1155
    pol = Policy(driver, AUTO, M=M)
    log = run_epochs(pol, 1200, lambda row, q, retry: 0.9 * M, hinted_after_first=True, frozen=False)
    pol.close()
    tried, started = set(), []
    for i, (pl, st) in enumerate(log):
        if pl is None:
            continue
        assert st["last_mean"] > 320                   # (more than `auto` bears, whatever ran)
        tried.add((st["hinted"], st["seed_full"], pl["planes"]))
        if st["filter_backoff"]:
            started.append(st["filter_backoff"])
            # ... then exactly that many all-pairs epochs, counting down
            after = log[i + 1:i + 1 + st["filter_backoff"]]      # (the last run is cut off by the end of the log)
            assert [s["filter_backoff"] for p, s in after] == list(range(st["filter_backoff"] - 1, -1, -1))[:len(after)]
            assert all(p is None for p, s in after)
        else:
            # no back-off although the lists are unbearable: only because an arm that has never run is up next
            # (arm 0 by a counting-only launch beside an arm that has)
            nxt = log[i + 1][0]
            assert nxt is not None
            assert nxt["probe"] or (1, nxt["seed_full"], nxt["planes"]) not in tried
    assert started[:7] == [8, 16, 32, 64, 128, 256, 256] and max(started) == 8 << 5


def clustered(row, q, retry):
    return {0: 30.0, 1: 42.0, 2: 27.0, 3: 22.0}[q] * (0.8 if row == 2 else 1.0)


def mid_clustered(row, q, retry):   # the triangle inequality leaves a third of the map, the sweeps short lists
    return {0: 400.0, 1: 42.0, 2: 27.0, 3: 26.0}[q]


def test_growth_within_a_quarter_keeps_what_is_known_and_a_larger_step_forgets_it(driver):
    """test_auto_policy_on_unclustered_data_and_across_a_growth_step: no second exploration after a small step."""
    pol = Policy(driver, FILTERED, M=1024)
    ms = lambda row, q: 2.0 + q   # noqa: E731
    log = run_epochs(pol, 30, mid_clustered, ms)
    assert log[0][0]["probe"] == 1                     # the first epoch of a map size always counts arm 0
    settled = log[-1][1]
    assert settled["plane_hold"] > 1 and settled["planes_next"] == 1 and settled["arm_ms"] == 3.0
    assert not pol.k2()                                # arm 0 left 400 of 1024: more than is borne
    pol.shape(1024 + 256, 160000, 784)                 # a quarter more: still the same map to the policy
    pl = pol.plan(bound=True)
    assert pl["probe"] == 1 and pl["planes"] == 1      # (arm 0 is counted again at every change of size)
    st = pol.observe(42.0, probe_lists=400.0)
    assert st["plane_hold"] == settled["plane_hold"] - 1 and st["planes_next"] == 1 and st["arm_ms"] == 3.0
    pl = pol.plan(bound=True)
    assert pl["probe"] == 0 and pl["planes"] == 1
    st = pol.observe(42.0, ms=3.5)
    assert st["plane_hold"] == settled["plane_hold"] - 2 and st["arm_ms"] == 3.25      # (the mean of the last two looks)
    pol.shape(1280 + 321, 160000, 784)                 # more than a quarter: another map, nothing is known of it
    pl = pol.plan(bound=True)
    assert pl["probe"] == 1 and pl["planes"] == 1
    st = pol.observe(42.0, probe_lists=30.0)
    assert st["plane_hold"] == 16 and st["planes_next"] == 0 and math.isnan(st["arm_ms"])
    assert pol.k2()                                    # arm 0 was counted on THIS map and left 30
    pol.close()


def test_long_lists_send_exploration_to_the_strong_corner_first(driver):
    """test_full_seed_prepass_on_weakly_clustered_data: on isotropic data no single step leads to (full seeds, two or
    three products) -- full seeds alone 1024 candidates, finer planes alone 981, both 17."""
    M = 1024

    def isotropic(row, q, retry):
        return {(0, 1): 1024.0, (0, 2): 981.0, (0, 3): 900.0, (1, 1): 1024.0, (1, 2): 17.0, (1, 3): 12.0}.get((row, q), float(M))

    pol = Policy(driver, FILTERED, M=M)
    log = run_epochs(pol, 12, isotropic)
    pol.close()
    assert (log[0][0]["seed_full"], log[0][0]["planes"]) == (0, 1)
    assert (log[1][0]["seed_full"], log[1][0]["planes"]) == (1, 2)       # straight to the corner
    assert log[1][0]["seed_stride"] & 0x100                               # DBGSOM_SEED_FULL
    assert log[-1][1]["plane_hold"] > 0 and log[-1][1]["seed_mode"] == 1 and log[-1][1]["planes_next"] in (2, 3)
    assert log[-1][1]["last_mean"] <= 17.0


@pytest.mark.parametrize("faster", [1, 2])
def test_two_timed_arms_are_compared_by_their_time_not_by_the_model(driver, faster):
    """test_search_arms_that_have_been_timed_are_compared_by_their_time: the model prices one product (lists 80) below
    two (lists 40), but not so far below that two products with empty lists would not be worth a look; once both
    have run clean, whichever the clock says is faster is kept."""
    pol = Policy(driver, FILTERED, M=1024)
    assert pol.cost(0, 2, 16.0) < pol.cost(0, 1, 80.0) < pol.cost(0, 2, 40.0)
    ms = lambda row, q: (3.0 if q == faster else 6.0) if q in (1, 2) else 50.0                             # noqa: E731
    lists = lambda row, q, retry: {0: 400.0, 1: 80.0, 2: 40.0, 3: 39.0}[q] if row == 0 else 1024.0         # noqa: E731
    log = run_epochs(pol, 40, lists, ms)
    pol.close()
    timed = {pl["planes"] for pl, st in log if pl["seed_full"] == 0 and not math.isnan(st["arm_ms"])}
    assert timed == {1, 2}
    assert log[-1][1]["plane_hold"] > 0 and log[-1][1]["planes_next"] == faster and log[-1][1]["seed_mode"] == 0
    assert [pl["planes"] for pl, st in log[-3:]] == [faster] * 3


def test_arm_zero_is_never_run_blind_only_probed(driver):
    """the pruning form runs only after a counting-only launch has shown what its lists would be"""
    for world in (clustered, lambda row, q, retry: 1024.0 if q == 0 else clustered(row, q, retry)):
        pol = Policy(driver, FILTERED_HINT, M=1024)
        log = run_epochs(pol, 40, world, lambda row, q: 2.0 + q, hinted_after_first=True)
        pol.close()
        counted = []
        for pl, st in log:
            if pl["planes"] == 0:
                assert counted and min(counted) <= 320 and pl["seed_stride"] & 0x200      # DBGSOM_PRUNE
            if pl["probe"]:
                assert pl["planes"] != 0 and pl["seed_stride"] & 0x400 and not math.isnan(st["probe_mean"])   # DBGSOM_PRUNE_PROBE
                counted.append(st["probe_mean"])
        assert log[0][0]["probe"] == 1
        ran0 = any(pl["planes"] == 0 for pl, st in log)
        assert ran0 == (world is clustered)      # lists of the whole map: counted, never run


def test_reseeding_turns_on_and_the_same_arm_is_measured_again(driver):
    """test_pruning_reseeds_workgroups_whose_cheap_seeds_missed_their_cluster"""
    pol = Policy(driver, FILTERED, M=1024)
    pl = pol.plan()
    assert pl["probe"] == 1 and pl["retry"] == 0 and pl["planes"] == 1
    st = pol.observe(42.0, probe_lists=70.0, retry_groups=25)      # cheap seeds left 25 workgroups with long lists
    assert st["prune_retry"] == 1 and st["probe_next"] == 1
    again = pol.plan(bound=True)
    assert (again["planes"], again["probe"], again["retry"]) == (pl["planes"], 1, 1)
    assert again["seed_stride"] & 0x800 and again["seed_stride"] & 0x400      # DBGSOM_PRUNE_RETRY | DBGSOM_PRUNE_PROBE
    st = pol.observe(42.0, probe_lists=30.0, retry_groups=25)      # they stay: that is what the arm costs on this data
    assert st["prune_retry"] == 1 and st["probe_mean"] == pytest.approx(30.0, rel=1e-3)
    nxt = pol.plan(bound=True)                                      # arm 0 itself, re-seeding on
    assert nxt["planes"] == 0 and nxt["retry"] == 1 and nxt["seed_stride"] & 0x200 and nxt["seed_stride"] & 0x800
    st = pol.observe(30.0, retry_groups=0, ms=2.0)
    assert st["prune_retry"] == 0 and st["arm_ms"] == 2.0          # ... and the flag does not keep the arm from being timed
    pol.close()


@pytest.mark.parametrize("with_ms, without_ms", [(4.0, 5.0), (5.0, 4.0)])
def test_refinement_is_timed_twice_per_form_on_a_settled_arm_and_chosen_by_the_smaller_time(driver, with_ms, without_ms):
    """test_refinement_is_chosen_by_measurement"""
    # an arm the caller fixed counts as settled
    pol = Policy(driver, FILTERED, M=1024, sweep_planes=2)
    forms = []
    for e in range(8):
        pl = pol.plan(bound=e > 0)
        forms.append((pl["timing_form"], pl["refine"]))
        if pl["timing_form"] >= 0:
            pol.refine_timed(pl["timing_form"], with_ms if pl["timing_form"] else without_ms)
        pol.observe(70.0)
    pol.close()
    keep = int(with_ms < without_ms)
    assert forms == [(-1, 0), (0, 0), (0, 0), (1, 1), (1, 1)] + [(-1, keep)] * 3
    # the adaptive policy: nothing is timed while it explores, only once it holds an arm
    pol = Policy(driver, FILTERED, M=1024)
    log = run_epochs(pol, 16, mid_clustered, lambda row, q: 3.0)
    pol.close()
    hold_before = [0] + [st["plane_hold"] for pl, st in log[:-1]]
    timing = [pl["timing_form"] for pl, st in log]
    assert all(h > 0 for h, t in zip(hold_before, timing) if t >= 0)
    assert [t for t in timing if t >= 0] == [0, 0, 1, 1]
    # few rows, few features or short lists: not eligible, never timed, never on
    for N, dp, mean in ((20000, 784, 70.0), (160000, 128, 70.0), (160000, 784, 12.0)):
        pol = Policy(driver, FILTERED, M=1024, N=N, dp=dp, sweep_planes=2)
        for e in range(6):
            pl = pol.plan(bound=e > 0)
            assert (pl["timing_form"], pl["refine"]) == (-1, 0)
            pol.observe(mean)
        pol.close()


# ------------------------------------------------------------------------------------------------------------------
# the mirror in backend.py
# ------------------------------------------------------------------------------------------------------------------
def header_constants(driver):
    out = subprocess.run([driver, "--constants"], capture_output=True, text=True, check=True).stdout
    vals = {}
    for line in out.splitlines():
        k, v = line.split()
        vals[k] = float.fromhex(v) if v.startswith("0x") or v.startswith("-0x") else int(v)
    return vals


def test_backend_mirrors_the_constants_of_the_header(driver):
    from dbgsom_amd import _native
    from dbgsom_amd.backend import HipBackend

    c = header_constants(driver)
    assert HipBackend.FILTER_MIN_PROTOTYPES == c["FILTER_MIN_PROTOTYPES"]
    assert HipBackend.FILTER_MAX_FEATURES == c["FILTER_MAX_FEATURES"] == 43690
    assert HipBackend.FILTER_MAX_MEAN_CANDIDATES == c["FILTER_MAX_MEAN_CANDIDATES"]
    assert _native.MAX_PROTOTYPES == c["MAX_PROTOTYPES"]
    assert HipBackend.SWEEP_COST == {q: c[f"SWEEP_COST_{q}"] for q in (1, 2, 3)}
    assert HipBackend.LIST_COST == c["LIST_COST"]
    assert HipBackend.PRUNE_PASS_COST == c["PRUNE_PASS_COST"]
    assert c["SEED_COST_2"] == 1.0      # plane_cost prices the hinted arms: seeds for free
    assert c["FILTER_BACKOFF"] == 8 and c["PLANES_REPROBE"] == 16 and c["PRUNE_MAX_M"] == 8192


@pytest.mark.parametrize("M, N, dp", [(1024, 160000, 784), (400, 6000, 64), (4096, 1000000, 784), (247, 1, 16),
                                      (16000, 50000, 43680)])
def test_plane_cost_is_the_policys_price_of_an_untimed_arm(driver, M, N, dp):
    from dbgsom_amd.backend import HipBackend

    pol = Policy(driver, FILTERED_HINT, M=M, N=N, dp=dp)
    for p in (0, 1, 2, 3):
        for mean in (0.0, 17.0, 33.25, 981.0):
            assert HipBackend.arm_cost(p, mean, M, N, dp) == pol.cost(2, p, mean), (p, mean)
    pol.close()
    # ... and plane_cost is that, for the resident samples
    be = object.__new__(type("B", (HipBackend,), {"padded_features": dp}))
    be._N = N
    assert be.plane_cost(0, 17.0, M) == HipBackend.arm_cost(0, 17.0, M, N, dp)
    assert be.plane_cost(2, 17.0, M) == HipBackend.arm_cost(2, 17.0, M, N, dp)
