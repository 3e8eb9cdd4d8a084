#!/bin/bash
# round 4: the evidence of the final build (GPU box) -> gpurun_out/r04_final/ (copied into profiles/r04/ afterwards)
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
O=gpurun_out/r04_final; mkdir -p $O
timeout 1800 python -m pytest tests -m gpu -x -q > $O/gpu_tests_final.txt 2>&1; tail -4 $O/gpu_tests_final.txt
timeout 900 python3 bench.py --full > $O/bench_final.json 2> $O/bench_final.err; echo "bench exit $?"
python3 - <<'PY'
import json
d = json.loads([l for l in open("gpurun_out/r04_final/bench_final.json") if l.startswith("{")][-1])
print({k: d[k] for k in ("value", "ms_per_step", "ms_per_align_alone", "ms_per_icp_iter_alone", "ms_per_icp_iter_amortised")})
print("roofline", {k: d["roofline"][k] for k in ("achieved", "frac", "avg_launch_us", "traffic")}, "step frac", d["step_roofline"]["frac"])
print("cpu", d.get("cpu_baseline", {}).get("value"), "pose delta", d.get("pose_delta_vs_cpu"))
for w in d["other_workloads"]:
    print(round(w["value"] / 1e9, 3), w.get("ms_per_step"), w.get("ms_per_align"), w.get("pairs_per_s_end_to_end"), w.get("pairs_per_s_align_only"), w["workload"][:90])
PY
# the whole bench under rocprofv3 (ticks as plain launches) + the accumulate launches of its roofline legs
bash tools/profile_bench.sh r04_final/r04 > $O/profile_bench.log 2>&1; tail -12 $O/profile_bench.log | cut -c1-220
# the timed region alone
rm -rf /tmp/tl_prof
SICP_NO_GRAPH=1 timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/tl_prof -- python3 bench.py --timed-only --steps 4 --warmup 1 > $O/bench_timed_only_under_rocprof.json 2> $O/bench_timed_only_under_rocprof.err
echo "timed-only under rocprofv3: exit $?"
f=$(find /tmp/tl_prof -name '*kernel_trace.csv' | head -1); s=$(find /tmp/tl_prof -name '*kernel_stats.csv' | head -1)
[ -n "$s" ] && cp "$s" $O/kernel_stats_timed_region.csv
[ -n "$f" ] && python3 tools/trace_timeline.py "$f" 10 700 > $O/timeline_timed_region.txt
# counters: HBM traffic of the accumulate launch, the search kernels
timeout 900 python3 tools/pmc_accumulate.py r04_final/r04 256 32 > $O/pmc_accumulate.log 2>&1; tail -3 $O/pmc_accumulate.log
timeout 1500 python3 tools/pmc_knn.py r04_final/r04 > $O/pmc_knn.log 2>&1; tail -3 $O/pmc_knn.log | cut -c1-300
ls $O
