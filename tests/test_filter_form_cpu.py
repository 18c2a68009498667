"""What a call of the filtered search resolves to (dbgsom_amd/csrc/filter_form.h) on the CPU: tests/filter_form_check.cpp
is compiled with the host C++ compiler.  The expected answers were derived by hand from launch_bmu_filtered as it stood
before the arithmetic moved into the header: the same conditions, the same messages.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_FULL, PRUNE, PRUNE_PROBE, PRUNE_RETRY = 0x100, 0x200, 0x400, 0x800
K2_MESSAGE = "k = 2 needs the pruning form (DBGSOM_PRUNE, M <= 8192) without the refinement"
FIELDS = ("seed_full", "prune", "prune_probe", "prune_retry", "k2", "seed_stride", "Msub", "Msubpad", "nkt_full",
          "nkt_used", "sweep_planes", "marking", "gap_nb", "refine", "rows0", "exact")


@pytest.fixture(scope="module")
def resolve(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler (c++ / g++) on PATH"
    exe = str(tmp_path_factory.mktemp("form") / "filter_form_check")
    # plain host C++: nothing of ROCm on the include path
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "dbgsom_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "filter_form_check.cpp")], check=True)

    def run(flags=0, planes=0, k=1, refine_rows=0, N=3000, d=32, M=1024, has_hint=False):
        line = f"{flags:#x} {planes} {k} {refine_rows} {N} {d} {M} {int(has_hint)}\n"
        out = subprocess.run([exe], input=line, capture_output=True, text=True, check=True).stdout.strip()
        head, _, rest = out.partition(" ")
        if head == "error":
            return rest
        assert head == "ok"
        vals = rest.split()
        assert len(vals) == len(FIELDS)
        return {k_: (v if k_ in ("marking", "exact") else int(v)) for k_, v in zip(FIELDS, vals)}

    return run


def test_header_is_host_only():
    text = open(os.path.join(ROOT, "dbgsom_amd", "csrc", "filter_form.h")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes == ["<stdint.h>", '"../../include/dbgsom_hip.h"']
    for word in ("hipStream_t", "hipError_t", "hip_runtime", "__global__", "__device__"):
        assert word not in text, word


def test_nothing_of_the_deferred_distance_path_is_left():
    """The sums kernel that also evaluated distances, its option and what threaded it through the search are gone
    ("The winner's distance inside this kernel"), and so is the option "graph" that selected nothing."""
    words = ("segsum_chain_kernel", "DistFill", "defer_dist", "defer_M", "n_active", "accumulate_can_fill_distances",
             "allow_defer", "last_deferred", "use_graph")
    sources = (".py", ".h", ".hip", ".cpp", ".sh", "Makefile")
    seen = 0
    for top in ("dbgsom_amd", "include", "tools"):
        for folder, _, names in os.walk(os.path.join(ROOT, top)):
            for name in names:
                if not name.endswith(sources) or (top == "tools" and name.startswith("probe_") and name.endswith(".hip")):
                    continue
                text = open(os.path.join(folder, name), encoding="utf-8").read()
                seen += 1
                for word in words:
                    assert word not in text, (os.path.join(folder, name), word)
    assert seen > 40   # (the walk found the sources)
    # the option and property names (backend.py's _QueryRows takes an unrelated `defer=` keyword)
    for path in (("include", "dbgsom_hip.h"), ("dbgsom_amd", "csrc", "engine.hip"), ("dbgsom_amd", "csrc", "filter_form.h")):
        text = open(os.path.join(ROOT, *path)).read()
        assert not re.search(r"\bdefer(_epochs)?\b", text), path
    text = open(os.path.join(ROOT, "dbgsom_amd", "backend.py")).read()
    assert not re.search(r"""["']defer(_epochs)?["']|^\s*defer(_epochs)?\s*=|\.defer(_epochs)?\b""", text, re.M)
    assert '"graph"' not in text


def test_flags_are_the_headers():
    text = open(os.path.join(ROOT, "include", "dbgsom_hip.h")).read()
    for name, value in (("SEED_FULL", SEED_FULL), ("PRUNE", PRUNE), ("PRUNE_PROBE", PRUNE_PROBE), ("PRUNE_RETRY", PRUNE_RETRY)):
        assert f"#define DBGSOM_{name} {value:#x}\n" in text


@pytest.mark.parametrize("flags, M, stride, Msub, Msubpad", [
    (0, 129, 1, 129, 256),          # default: ceil(M / 256), at least 4 -- then halved until 128 prototypes are left
    (0, 300, 2, 150, 256),
    (0, 700, 4, 175, 256),
    (0, 1024, 4, 256, 256),
    (0, 8192, 32, 256, 256),
    (0, 16000, 63, 254, 256),
    (64, 200, 1, 200, 256),         # the caller's stride is halved the same way
    (8, 4096, 8, 512, 512),
    (1, 4096, 1, 4096, 4096),
    (SEED_FULL, 1024, 1, 1024, 1024),
    (SEED_FULL | 16, 1024, 1, 1024, 1024),
])
def test_seed_stride_and_the_subset_of_the_prepass(resolve, flags, M, stride, Msub, Msubpad):
    f = resolve(flags=flags, M=M)
    assert (f["seed_stride"], f["Msub"], f["Msubpad"]) == (stride, Msub, Msubpad)
    assert f["seed_full"] == int(bool(flags & SEED_FULL))


def test_k_tiles_of_the_prepass(resolve):
    # d = 784: 13 k-tiles of 64 features, three of them unless the seeds are full
    assert (resolve(d=784)["nkt_full"], resolve(d=784)["nkt_used"]) == (13, 3)
    assert (resolve(flags=SEED_FULL, d=784)["nkt_full"], resolve(flags=SEED_FULL, d=784)["nkt_used"]) == (13, 13)
    # rows are padded to two k-tiles at least; three tiles or fewer: all of them
    assert (resolve(d=16)["nkt_full"], resolve(d=16)["nkt_used"]) == (2, 2)
    assert (resolve(d=192)["nkt_full"], resolve(d=192)["nkt_used"]) == (3, 3)
    assert (resolve(d=208)["nkt_full"], resolve(d=208)["nkt_used"]) == (4, 3)
    # more tiles than the selection handles (1024): all of them
    assert (resolve(d=65536)["nkt_full"], resolve(d=65536)["nkt_used"]) == (1024, 3)
    assert (resolve(d=65537)["nkt_full"], resolve(d=65537)["nkt_used"]) == (1025, 1025)


def test_pruning_flags(resolve):
    f = resolve(flags=PRUNE, M=8192)
    assert (f["prune"], f["prune_probe"], f["marking"], f["gap_nb"]) == (1, 0, "prune", 2)
    f = resolve(flags=PRUNE, M=8193)                     # beyond the gap matrix: ignored
    assert (f["prune"], f["prune_probe"], f["marking"], f["gap_nb"]) == (0, 0, "sweep_2_2", 0)
    f = resolve(flags=PRUNE_PROBE, M=8192, planes=1)
    assert (f["prune"], f["prune_probe"], f["marking"], f["gap_nb"]) == (0, 1, "sweep4", 2)
    assert resolve(flags=PRUNE_PROBE, M=8193)["prune_probe"] == 0
    f = resolve(flags=PRUNE | PRUNE_PROBE)               # the pruning form itself: nothing to probe
    assert (f["prune"], f["prune_probe"]) == (1, 0)
    # re-seeding: stateless searches with cheap seeds only
    assert resolve(flags=PRUNE | PRUNE_RETRY)["prune_retry"] == 1
    assert resolve(flags=PRUNE_PROBE | PRUNE_RETRY)["prune_retry"] == 1
    assert resolve(flags=PRUNE | PRUNE_RETRY, has_hint=True)["prune_retry"] == 0
    assert resolve(flags=PRUNE | PRUNE_RETRY | SEED_FULL)["prune_retry"] == 0
    # the flags are no part of the stride
    assert resolve(flags=PRUNE | PRUNE_PROBE | PRUNE_RETRY | 8, M=4096)["seed_stride"] == 8


@pytest.mark.parametrize("flags", [PRUNE, PRUNE_PROBE])
def test_gap_kernel_form_switches_at_four_tiles_per_cu(resolve, flags):
    # Mg = M rounded up to 64; 64 x 64 tiles once (Mg / 64)^2 >= 1024
    assert resolve(flags=flags, M=1984)["gap_nb"] == 1   # Mg 1984: 31 x 31 tiles
    assert resolve(flags=flags, M=1985)["gap_nb"] == 2   # Mg 2048: 32 x 32
    assert resolve(flags=flags, M=2048)["gap_nb"] == 2
    assert resolve(flags=flags, M=2)["gap_nb"] == 1
    assert resolve(flags=0, M=2048)["gap_nb"] == 0


def test_two_nearest_prototypes_need_the_pruning_form(resolve):
    assert resolve(k=2) == K2_MESSAGE
    assert resolve(k=2, flags=PRUNE_PROBE) == K2_MESSAGE
    assert resolve(k=2, flags=PRUNE, M=8193) == K2_MESSAGE
    assert resolve(k=2, flags=PRUNE, refine_rows=192) == K2_MESSAGE
    assert resolve(k=2, flags=PRUNE, M=1) == K2_MESSAGE
    f = resolve(k=2, flags=PRUNE, M=2)
    assert (f["k2"], f["prune"], f["marking"], f["exact"]) == (1, 1, "prune", "k2")
    assert resolve(k=2, flags=PRUNE, N=10 ** 6)["exact"] == "k2"
    assert resolve(k=0) == "k must be 1 or 2" and resolve(k=3, flags=PRUNE) == "k must be 1 or 2"


def test_rejected_options(resolve):
    assert resolve(flags=65) == "seed_stride outside [0, 64]"
    assert resolve(flags=0x1000) == "seed_stride outside [0, 64]"        # (DBGSOM_REFINE is the ABI wrapper's to strip)
    assert resolve(flags=SEED_FULL | 65)["seed_stride"] == 1              # (full seeds: the stride is not looked at)
    assert resolve(planes=4) == "sweep_planes must be 0 .. 3" and resolve(planes=-1) == "sweep_planes must be 0 .. 3"
    # the order of the checks: k, k = 2, stride, planes
    assert resolve(k=3, flags=65, planes=4) == "k must be 1 or 2"
    assert resolve(k=2, flags=65, planes=4) == K2_MESSAGE
    assert resolve(flags=65, planes=4) == "seed_stride outside [0, 64]"


@pytest.mark.parametrize("planes, M, marking, resolved", [
    (1, 8192, "sweep4", 1),          # one product: two workgroups per CU while the bitmask holds the map
    (1, 8193, "sweep_1_4", 1),
    (1, 16000, "sweep_1_4", 1),
    (1, 1, "sweep4", 1),
    (0, 1024, "sweep_2_2", 2),       # default: two planes
    (2, 9000, "sweep_2_2", 2),
    (3, 1024, "sweep_3_1", 3),
    (3, 9000, "sweep_3_1", 3),
])
def test_candidate_kernel(resolve, planes, M, marking, resolved):
    f = resolve(planes=planes, M=M)
    assert (f["marking"], f["sweep_planes"]) == (marking, resolved)
    assert resolve(planes=planes, M=M, flags=PRUNE_PROBE)["marking"] == marking
    assert resolve(planes=planes, M=M, flags=PRUNE)["marking"] == ("prune" if M <= 8192 else marking)


@pytest.mark.parametrize("refine_rows, rows0", [(1, 32), (32, 32), (33, 64), (64, 64), (65, 128), (128, 128), (129, 0),
                                                (192, 0)])
def test_small_tile_of_the_refinement(resolve, refine_rows, rows0):
    f = resolve(refine_rows=refine_rows)
    assert (f["refine"], f["rows0"], f["exact"]) == (1, rows0, "beside_refine")


def test_exact_stage_form(resolve):
    assert resolve(N=1024 * 128)["exact"] == "split"          # nb = 1024
    assert resolve(N=1024 * 128 + 1)["exact"] == "all"        # nb = 1025
    assert resolve(N=1)["exact"] == "split"
    assert resolve(N=1024 * 128 + 1, refine_rows=64)["exact"] == "beside_refine"
    assert resolve(N=1, refine_rows=64)["exact"] == "beside_refine"
    assert resolve(refine_rows=0)["refine"] == 0
