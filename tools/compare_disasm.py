"""Kernel-by-kernel comparison of two `llvm-objdump -d` listings of device code (addresses and encodings
dropped, names demangled with c++filt, trailing padding ignored): which kernels are instruction for
instruction the same, which differ (first lines of the diff with -v), which exist on one side only.
`--strip TEXT` removes TEXT from the demangled names first (a template argument one side gained); `--rename OLD=NEW`
then replaces OLD by NEW in them, on both sides (a kernel that got another name: its old name becomes its new one).
    hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=on --cuda-device-only --no-gpu-bundle-output \\
          -c accumulate.hip -o new.co && llvm-objdump -d new.co > new.dis
    python tools/compare_disasm.py old.dis new.dis --strip ", dbgsom::WeightArg<false>" --strip ", false" --strip "<false>"
    python tools/compare_disasm.py old.dis new.dis --strip "dbgsom::AbsTerm, dbgsom::PlainFinish, " \\
          --rename ", dbgsom::PlainFinish)=)" --rename l1_bmu_kernel=direct_bmu_kernel """
import argparse
import difflib
import re
import subprocess


def parse(path, strips, renames=()):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
        if m:
            cur = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            for t in strips:
                cur = cur.replace(t, "")
            for old, new in renames:
                cur = cur.replace(old, new)
            cur = re.sub(r"^void\s+", "", re.sub(r"\s+", " ", cur))
            out[cur] = []
        elif cur and line.strip():
            out[cur].append(re.sub(r"^[0-9a-f]+:\s*", "", line.split("//")[0].strip()))
    for body in out.values():
        while body and body[-1] in ("s_nop 0", "..."):
            body.pop()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--strip", action="append", default=[])
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("-v", action="store_true")
    args = ap.parse_args()
    renames = [tuple(r.split("=", 1)) for r in args.rename]
    a, b = parse(args.old, args.strip, renames), parse(args.new, args.strip, renames)
    for k in a:
        if k not in b:
            print("ONLY OLD ", k)
            continue
        same = a[k] == b[k]
        print("same     " if same else "DIFFERENT", k, len(a[k]), len(b[k]))
        if args.v and not same:
            for line in list(difflib.unified_diff(a[k], b[k], lineterm="", n=0))[:40]:
                print("    ", line)
    for k in b:
        if k not in a:
            print("ONLY NEW ", k)


if __name__ == "__main__":
    main()
