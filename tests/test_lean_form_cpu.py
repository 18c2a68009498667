"""CPU: the lean form of the anchor-marked search.  Which calls take it (FilterForm::lists_only, filter_form.h), what it
launches and no longer needs, and when the engine asks for it (LeanGate, lean_gate.h) -- both through
tests/lean_form_check.cpp, compiled with the host C++ compiler.

The lean form is valid on exactly the calls whose lists anchor_mark_kernel writes (stateless, k = 1, DBGSOM_PRUNE, anchor
buckets with their run table) as long as nothing behind that kernel reads the digit planes of W: no re-seeding pass, no
refinement.  Everywhere else the bit is ignored and the form is what it is without the bit."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_FULL, PRUNE, PRUNE_PROBE, PRUNE_RETRY, LISTS_ONLY = 0x100, 0x200, 0x400, 0x800, 0x2000
FIELDS = ("lists_only", "anchor_mark", "w_planes", "gap_nb", "prune_retry", "refine", "seed_stride", "marking", "exact")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler (c++ / g++) on PATH"
    exe = str(tmp_path_factory.mktemp("lean_form") / "lean_form_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "dbgsom_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "lean_form_check.cpp")], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, check=True)
        answers = out.stdout.splitlines()
        assert len(answers) == len(lines), (lines, answers)
        return answers

    return run


def _form(check, flags=PRUNE, planes=0, k=1, refine_rows=0, M=1024, has_hint=False, anchors=True, runs=True):
    out = check([f"form {flags:#x} {planes} {k} {refine_rows} {M} {int(has_hint)} {int(anchors)} {int(runs)}"])[0]
    head, _, rest = out.partition(" ")
    if head == "error":
        return rest
    vals = rest.split()
    form = {name: (v if name in ("marking", "exact") else int(v)) for name, v in zip(FIELDS, vals)}
    form["passes"] = vals[len(FIELDS):]
    return form


def test_headers_are_host_only():
    text = open(os.path.join(ROOT, "dbgsom_amd", "csrc", "lean_gate.h")).read()
    assert [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")] == ["<stdint.h>"]
    for word in ("hipStream_t", "hipError_t", "hip_runtime", "__global__", "__device__"):
        assert word not in text, word
    assert f"#define DBGSOM_ANCHOR_LISTS_ONLY {LISTS_ONLY:#x}\n" in open(os.path.join(ROOT, "include", "dbgsom_hip.h")).read()


def test_the_lean_form_launches_anchor_mark_and_nothing_else(check):
    f = _form(check, flags=PRUNE | LISTS_ONLY)
    assert f["lists_only"] == 1 and f["anchor_mark"] == 1
    assert f["passes"] == ["anchor_mark"]
    assert f["w_planes"] == 0 and f["gap_nb"] == 0          # no digit planes of W, no gap table
    # the same call without the bit: the planes, the gaps and the per-sample pass behind the anchors' lists
    g = _form(check, flags=PRUNE)
    assert (f["marking"], f["exact"]) == ("prune", "split") == (g["marking"], g["exact"])   # no sweep; the exact stage as ever
    assert g["lists_only"] == 0 and g["w_planes"] == 1 and g["gap_nb"] == 1 and g["passes"] == ["anchor_mark", "prune_handed"]
    assert _form(check, flags=PRUNE | LISTS_ONLY, M=2048)["gap_nb"] == 0 and _form(check, flags=PRUNE, M=2048)["gap_nb"] == 2


def test_the_bit_is_no_part_of_the_stride(check):
    assert _form(check, flags=PRUNE | LISTS_ONLY | 8, M=4096)["seed_stride"] == 8
    assert _form(check, flags=LISTS_ONLY | 8, M=4096, anchors=False, runs=False)["seed_stride"] == 8
    assert _form(check, flags=LISTS_ONLY | 65) == "seed_stride outside [0, 64]"


CASES = list(itertools.product((PRUNE, PRUNE | PRUNE_RETRY, PRUNE | SEED_FULL, PRUNE_PROBE, 0),   # flags
                               (1, 2),                    # k
                               (0, 64),                   # refine_rows
                               (False, True),             # has_hint
                               ((False, False), (True, False), (True, True)),   # anchors, run table
                               (1024, 8193)))             # M (beyond 8192: no pruning form)


def test_the_member_is_set_exactly_where_the_form_is_valid_and_nothing_else_changes(check):
    lines, expect = [], []
    for flags, k, refine_rows, hint, (anchors, runs), M in CASES:
        planes = 1 if flags in (PRUNE_PROBE, 0) else 0
        for bit in (0, LISTS_ONLY):
            lines.append(f"form {flags | bit:#x} {planes} {k} {refine_rows} {M} {int(hint)} {int(anchors)} {int(runs)}")
        prune = bool(flags & PRUNE) and M <= 8192
        retry = bool(flags & PRUNE_RETRY) and not (flags & SEED_FULL) and not hint
        anchor_mark = prune and anchors and runs and k == 1 and not hint and not (flags & SEED_FULL)
        expect.append(anchor_mark and not retry and refine_rows == 0 and k == 1)
    answers = check(lines)
    n_lean = 0
    for (plain, with_bit), lean, case in zip(zip(answers[0::2], answers[1::2]), expect, CASES):
        if plain.startswith("error"):
            assert with_bit == plain, case                   # rejected alike
            continue
        words = with_bit.split()
        assert words[0] == "ok" and int(words[1]) == int(lean), (case, with_bit)
        if not lean:
            assert with_bit == plain, case                   # the bit is ignored: today's form
        else:
            n_lean += 1
            assert plain.split()[1] == "0" and words[len(FIELDS) + 1:] == ["anchor_mark"], (case, with_bit)
    assert n_lean == 1       # of all these: stateless k = 1 DBGSOM_PRUNE with anchors and table, no retry, no refinement


def test_the_engine_asks_only_behind_a_clean_anchor_seeded_epoch(check):
    key = check(["key 0x204 0", "key 0xa04 0", "key 0x204 1"])
    assert len(set(key)) == 3                                # the plan's flags and planes tell plans apart
    k = key[0]
    script = [
        (f"allows 1024 1 {k} 0 0", "0"),                     # nothing known yet: a full epoch
        (f"record 1024 1 {k} 0 0", "recorded"),              # ... which handed nothing over and left nothing long
        (f"allows 1024 1 {k} 0 0", "1"),
        (f"allows 1024 1 {k} 1 0", "0"),                     # the plan re-seeds
        (f"allows 1024 1 {k} 0 1", "0"),                     # the plan refines
        (f"allows 1025 1 {k} 0 0", "0"),                     # a growth step
        (f"allows 1024 2 {k} 0 0", "0"),                     # a new load / rebuilt or dropped buckets
        (f"allows 1024 1 {key[2]} 0 0", "0"),                # another plan
        (f"record 1024 1 {k} 0 0", "recorded"),              # a lean epoch that kept no long list
        (f"allows 1024 1 {k} 0 0", "1"),
        (f"record 1024 1 {k} 3 0", "recorded"),              # a lean epoch that kept three: a wrong guess
        (f"allows 1024 1 {k} 0 0", "0"),
        (f"record 1024 1 {k} 3 0", "recorded"),              # the full epoch behind it handed them over, settled them
        (f"allows 1024 1 {k} 0 0", "0"),
        (f"record 1024 1 {k} 0 2", "recorded"),              # long lists behind the per-sample pass
        (f"allows 1024 1 {k} 0 0", "0"),
        (f"record 1024 1 {k} 0 0", "recorded"),
        (f"allows 1024 1 {k} 0 0", "1"),
        ("forget", "forgotten"),                             # an epoch that was hinted, unfiltered or pre-pass seeded
        (f"allows 1024 1 {k} 0 0", "0"),
        (f"record 1024 1 {k} nan 0", "recorded"),            # counts that are not numbers are no evidence
        (f"allows 1024 1 {k} 0 0", "0"),
    ]
    assert check([cmd for cmd, _ in script]) == [ans for _, ans in script]
