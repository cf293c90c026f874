#!/bin/bash
# Round-end evidence: kernel stats of the default bench (timeout 600 rocprofv3 --kernel-trace --stats) + HBM traffic PMC passes.
#   bash tools/round_profile.sh r01 <out dir>   -> <out dir>/{r01_kernel_stats.csv, r01_bench.json}; traffic: collect_traffic.sh
R=${GRAFT_REPO_ROOT:-$(pwd)}
TAG=${1:-r01}
OUT=$(realpath "${2:?usage: round_profile.sh <tag> <out dir>}")
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
rm -rf "$OUT/prof_$TAG"
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_$TAG" -- python3 $R/bench.py --full --no-cpu-baseline --no-extras --no-calibration > "$OUT/${TAG}_bench_under_rocprof.log" 2>&1
f=$(find "$OUT/prof_$TAG" -name "*kernel_stats.csv" | head -1)
cp "$f" "$OUT/${TAG}_kernel_stats.csv"
python3 $R/bench.py --full 2>/dev/null | tail -1 > "$OUT/${TAG}_bench.json"
bash $R/tools/collect_traffic.sh $TAG
bash $R/tools/collect_valu.sh $TAG
head -8 "$OUT/${TAG}_kernel_stats.csv"
cat "$OUT/${TAG}_bench.json" | cut -c1-600
