# The end-of-round check in one command: the GPU suite, smoke(), the plain bench line and the --full one.
#   bash tools/final_check.sh OUT_DIR
# Every step has a time limit of its own; the first failure ends the script with its status.
O=${1:?usage: bash tools/final_check.sh OUT_DIR}
mkdir -p "$O"
exec 3>&1   # (the steps' own output goes to their logs)
run() { "$@"; rc=$?; if [ $rc -ne 0 ]; then echo "final_check: '$*' failed ($rc)" >&3; exit $rc; fi; }
run timeout -k 10 900 python -m pytest tests -m gpu -x -q > "$O/gpu.log" 2>&1
tail -1 "$O/gpu.log"
run timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$O/smoke.log" 2>&1
tail -1 "$O/smoke.log"
run timeout -k 10 300 python bench.py > "$O/bench.json" 2> "$O/bench.err"
run timeout -k 10 600 python bench.py --full > "$O/bench_full.json" 2> "$O/bench_full.err"
python - "$O" <<'PY'
import json, sys
line = lambda name: json.loads(open(sys.argv[1] + "/" + name).read().strip().split("\n")[-1])
j, f = line("bench.json"), line("bench_full.json")
print(j["metric"], round(j["value"]/1e6,1), round(j["ms_per_step"],4))
print("--full:", round(f["value"]/1e6,1), round(f["ms_per_step"],4), round(f["roofline"]["frac"],3), f["roofline"]["traffic"], f["parity"]["ok"], round(f["cpu_baseline"]["value"]))
PY
