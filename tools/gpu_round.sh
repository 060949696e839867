# One GPU session: GPU tests, smoke, the full bench line (bench.py --full), a kernel-trace profile
# of the same bench with the timed-region statistics.  Every GPU step has its own time limit; the
# first failure ends the script (set -e).  Output goes to $1 (default build/gpu_round).
set -e
OUT=${1:-build/gpu_round}
mkdir -p "$OUT"
export TMPDIR=/tmp
python - > "$OUT/host.txt" <<'PY'
import os
print("os.cpu_count", os.cpu_count(), "affinity", len(os.sched_getaffinity(0)))
for f in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/memory.max"):
    try:
        print(f, open(f).read().strip())
    except OSError as e:
        print(f, e)
PY
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread ${PYTEST_ARGS:-} > "$OUT/pytest_gpu.log" 2>&1
tail -3 "$OUT/pytest_gpu.log"
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1
timeout -k 10 500 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -o run -- python3 bench.py --full --no-cpu --no-pmc > "$OUT/bench_prof.json" 2> "$OUT/bench_prof.err"
python tools/timed_region_stats.py "$OUT/prof" "$OUT/bench_prof.json" "$OUT/timed_region_stats.txt"
cat "$OUT/smoke.log" "$OUT/bench.json"
