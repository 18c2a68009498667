"""CPU: the engine-side control of the resident k = 1 search (AnchorControl, ResidentSearchState: csrc/epoch_control.h)
through tests/epoch_control_check.cpp, compiled with the host C++ compiler.

The driver holds the text the header replaced -- the inline logic of engine.hip at commit 2d7f700, transcribed as
`legacy_*` functions over a struct of the old fields -- and requires the same fields and answers from the new structs:
over every input of the two decisions (`enumerate`) and over event sequences in lockstep (`sequences`).  The scenarios
restate without a GPU what tests/test_gpu_lean_anchor_epoch.py asserts about the control."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dbgsom_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler (c++ / g++) on PATH"
    path = str(tmp_path_factory.mktemp("epoch_control") / "epoch_control_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", path,
                    os.path.join(ROOT, "tests", "epoch_control_check.cpp")], check=True)
    return path


def _counts(exe, mode):
    out = subprocess.run([exe, mode], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    print(out.stdout)
    return {name: int(value) for name, value in (ln.split() for ln in out.stdout.splitlines())}


def _scenario(exe, script):
    """script: [(command, expected answer)]; an epoch answers "seeded lean clean drop anchor_state" """
    out = subprocess.run([exe, "scenario"], input="".join(cmd + "\n" for cmd, _ in script), capture_output=True, text=True,
                         check=True)
    assert out.stdout.splitlines() == [ans for _, ans in script]


def test_header_is_host_only():
    text = open(os.path.join(CSRC, "epoch_control.h")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes == ["<math.h>", "<stdint.h>", '"../../include/dbgsom_hip.h"', '"lean_gate.h"', '"search_policy.h"']
    for word in ("hipStream_t", "hipError_t", "DevBuf", "dbgsom_ctx *", "hip_runtime", "__global__", "__device__", "chrono"):
        assert word not in text, word


MOVED = ("hint_valid", "hintM", "last_idx_valid", "dist_bound_valid", "distW_buf", "distW_M", "last_anchor_seeded", "last_lean",
         "last_plan_key", "anchors_built_now", "prepass_mean", "prepass_M")


def test_the_header_is_the_only_place_the_moved_fields_change():
    import re

    text = open(os.path.join(CSRC, "engine.hip")).read()
    for name in MOVED:
        hits = re.findall(r"[^\n]*\b%s\s*(?:=[^=]|\+\+|--|[-+|&^]=)[^\n]*" % name, text)
        assert not hits, (name, hits)
    assert "lean_gate." not in text and '"epoch_control.h"' in text


def test_every_decision_is_the_parents(exe):
    n = _counts(exe, "enumerate")
    # the comparison reached every branch: on the order of 10^5 inputs per decision, and each outcome among them
    assert n["before_search"] >= 100000 and n["after_filtered_epoch"] >= 100000
    for branch in ("anchor_seeded", "lean", "built", "clean_true", "clean_false", "valve_fired", "valve_not_fired",
                   "reference_taken", "probe_reference_taken", "lean_missed"):
        assert n[branch] > 0, branch
    assert n["anchor_seeded"] < n["before_search"] and n["lean"] < n["anchor_seeded"]
    assert n["clean_true"] + n["clean_false"] == n["after_filtered_epoch"] == n["valve_fired"] + n["valve_not_fired"]


def test_event_sequences_in_lockstep(exe):
    n = _counts(exe, "sequences")
    # every sequence of up to 5 events (16 of the search state, 13 of the anchor control), 4000 random ones of 30
    assert n["state_steps"] == sum(k * 16 ** k for k in range(1, 6)) + 4000 * 30
    assert n["anchor_steps"] == sum(k * 13 ** k for k in range(1, 6)) + 4000 * 30
    for branch in ("anchor_seeded", "lean", "dropped", "random_anchor_seeded", "random_lean", "random_dropped"):
        assert n[branch] > 0, branch


# ------------------------------------------------------------------------------------------------------------------
# scenarios: epochs of the pruning arm on the cheap seeds, M prototypes, 4096 samples
# ------------------------------------------------------------------------------------------------------------------
PREPASS = ("epoch 130 10 0 0", "0 0 1 0 0")    # the pre-pass seeds the reference epoch
BUILT = ("epoch 130 10 0 0", "1 0 0 0 1")      # anchors: built on the way (no clean clock), a full epoch
LEAN = ("epoch 130 10 0 0", "1 1 1 0 1")


def test_the_first_anchor_seeded_epoch_is_full_and_the_next_ones_lean(exe):
    _scenario(exe, [PREPASS, BUILT, LEAN, LEAN, LEAN])


def test_never_lean_while_lists_are_handed_over(exe):
    handed = ("epoch 130 10 0 32", "1 0 1 0 1")
    _scenario(exe, [PREPASS, ("epoch 130 10 0 32", "1 0 0 0 1"), handed, handed, handed, handed])
    # ... nor behind long lists left by the per-sample pass (the policy turns re-seeding on: not a settled epoch)
    _scenario(exe, [PREPASS, BUILT, LEAN, ("epoch 130 10 2 0", "1 1 1 0 1"), ("epoch 130 10 0 0", "1 0 1 0 1"), LEAN])


def test_a_wrong_guess_makes_the_next_epoch_full(exe):
    _scenario(exe, [
        PREPASS, BUILT, LEAN,
        # every list the whole map: the guess is made, its long lists are kept (handed: 32 workgroups), the clock is
        # not the arm's and the lists are not held against the valve
        ("epoch 130 130 0 32", "1 1 0 0 1"),
        ("epoch 130 10 0 0", "1 0 1 0 1"),     # the epoch behind a wrong guess is a full one
        LEAN,
    ])


def test_growth_and_reload_start_from_a_full_epoch(exe):
    _scenario(exe, [
        PREPASS, BUILT, LEAN,
        ("epoch 131 10 0 0", "1 0 1 0 1"),     # one more prototype: seeded from the anchors at once, full
        ("epoch 131 10 0 0", "1 1 1 0 1"),
        ("load", "loaded"),
        PREPASS,                               # the reference went with the samples
        BUILT,                                 # other buckets: the first anchor-seeded epoch is a full one
        LEAN,
        ("epoch 200 10 0 0", "0 0 1 0 1"),     # a map more than a quarter larger: the pre-pass seeds a new reference
        ("epoch 200 10 0 0", "1 0 1 0 1"),
    ])


def test_the_valve_drops_the_anchors_above_1_25_and_not_at_1_25(exe):
    _scenario(exe, [PREPASS, BUILT, ("epoch 130 12.5 0 0", "1 1 1 0 1"), ("epoch 130 12.5 0 0", "1 1 1 0 1")])
    _scenario(exe, [
        PREPASS, BUILT,
        ("epoch 130 12.500001 0 0", "1 1 1 1 2"),
        ("epoch 130 10 0 0", "0 0 1 0 2"),     # dropped for this sample set: the pre-pass seeds it again ...
        ("load", "loaded"),
        PREPASS, BUILT, LEAN,                  # ... until the next load
    ])
    # an epoch whose long lists the policy is about to re-seed is not held against the valve
    _scenario(exe, [PREPASS, BUILT, ("epoch 130 100 3 0", "1 1 1 0 1")])
