"""CPU: which calls take their candidate lists from the anchors, which passes they launch (dbgsom_amd/csrc/filter_form.h,
through tests/anchor_form_check.cpp), and what the search policy (search_policy.h, through tests/policy_replay.cpp) makes
of the counts those passes report.

anchor_mark_kernel hands workgroups with long lists to prune_mark_kernel's per-sample pass.  The count the policy reads
("workgroups whose pruned lists came out long", which turns the re-seeding passes on) must mean what it meant when
prune_mark_kernel ran over the whole grid: lists that are long AFTER the per-sample pass.  A hand-over is no such list,
so anchor_mark_kernel is not among the passes that report, and an epoch in which it handed workgroups over but the
per-sample pass settled them all leaves the re-seeding off."""
import os
import shutil
import subprocess

import pytest

from tests import test_search_policy_cpu as tsp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_FULL, PRUNE, PRUNE_PROBE, PRUNE_RETRY = 0x100, 0x200, 0x400, 0x800


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler (c++ / g++) on PATH"
    return cxx


@pytest.fixture(scope="module")
def passes(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("anchor_form") / "anchor_form_check")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "dbgsom_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "anchor_form_check.cpp")], check=True)

    def run(flags=PRUNE, planes=0, k=1, refine_rows=0, M=1024, has_hint=False, anchors=True, runs=True):
        line = f"{flags} {planes} {k} {refine_rows} {M} {int(has_hint)} {int(anchors)} {int(runs)}\n"
        out = subprocess.run([exe], input=line, capture_output=True, text=True, check=True).stdout.strip()
        assert out.startswith("ok "), out
        head, reports = out[3:].split(" | reports:")
        words = head.split()
        return bool(int(words[0])), words[1:], reports.split()

    return run


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("policy_anchor") / "policy_replay")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "dbgsom_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "policy_replay.cpp")], check=True)
    return exe


def test_the_form_applies_to_stateless_k1_pruning_calls_with_anchors_and_table(passes):
    assert passes() == (True, ["anchor_mark", "prune_handed"], ["prune_handed"])
    assert passes(flags=PRUNE | PRUNE_RETRY) == (True, ["anchor_mark", "prune_handed", "reseed", "prune_reseeded"], ["prune_handed"])
    # everything else takes the path it took
    grid = (False, ["prune_grid"], ["prune_grid"])
    assert passes(runs=False) == grid                                   # anchors without a table
    assert passes(anchors=False, runs=False) == grid
    assert passes(anchors=False, runs=True) == grid                     # (a table alone: the launcher rejects the call)
    assert passes(has_hint=True) == grid                                # hinted
    assert passes(k=2, M=1024) == grid                                  # the two nearest
    assert passes(flags=PRUNE | SEED_FULL) == grid                      # (full seeds: the launcher rejects anchors there)
    assert passes(flags=PRUNE_PROBE, planes=1) == grid                  # the counting-only probe beside a sweep
    assert passes(flags=PRUNE | PRUNE_RETRY, runs=False) == (False, ["prune_grid", "reseed", "prune_reseeded"], ["prune_grid"])
    assert passes(flags=PRUNE | PRUNE_RETRY, has_hint=True) == grid     # (hinted: no re-seeding)
    assert passes(flags=0, planes=1) == (False, [], [])                 # a sweep: no pruning pass at all
    assert passes(flags=PRUNE, M=8193) == (False, [], [])               # beyond the gap matrix: the sweep


def test_a_hand_over_is_never_reported_as_a_long_list(passes):
    for flags in (PRUNE, PRUNE | PRUNE_RETRY):
        on, launched, reports = passes(flags=flags)
        assert on and launched[0] == "anchor_mark" and "anchor_mark" not in reports
        assert reports == ["prune_handed"] and launched.index("prune_handed") == 1


def _settled_pruning_policy(driver):
    """a policy on the stateless pruning arm (sweep_planes = 4) whose first epoch left short lists and none long"""
    pol = tsp.Policy(driver, tsp.FILTERED, sweep_planes=4, seed_stride=4)
    assert pol.allowed()
    pl = pol.plan()
    assert pl["planes"] == 0 and not pl["retry"] and pl["seed_stride"] & PRUNE and not pl["seed_stride"] & PRUNE_RETRY
    st = pol.observe(40.0, retry_groups=0)
    assert not st["prune_retry"]
    return pol


def test_handed_workgroups_the_per_sample_pass_settled_leave_the_reseeding_off(driver):
    """what the engine observes of such an epoch: the per-sample pass (the reporting pass) counted no long list"""
    pol = _settled_pruning_policy(driver)
    for _ in range(3):
        pl = pol.plan()
        assert not pl["retry"] and not pl["seed_stride"] & PRUNE_RETRY
        st = pol.observe(40.0, retry_groups=0)
        assert not st["prune_retry"] and st["planes_used"] == 0
    pol.close()


def test_lists_still_long_after_the_per_sample_pass_turn_it_on_and_off_again(driver):
    pol = _settled_pruning_policy(driver)
    pol.plan()
    st = pol.observe(60.0, retry_groups=7)                # seven workgroups long after the per-sample pass
    assert st["prune_retry"]
    pl = pol.plan()
    assert pl["retry"] and pl["seed_stride"] & PRUNE_RETRY
    st = pol.observe(45.0, retry_groups=7)                # (with the passes on: the workgroups that were re-seeded)
    assert st["prune_retry"]
    pol.plan()
    st = pol.observe(40.0, retry_groups=0)
    assert not st["prune_retry"]
    pol.close()
