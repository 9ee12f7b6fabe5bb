#!/bin/bash
# rocprofv3 kernel-trace summary of one `bench.py --full` run on the default workload (C3, end to end, resident passes included).
# Usage: tools/profile.sh <tag> [extra bench.py arguments]    results: $PROFILE_OUT/prof_<tag>* (default PROFILE_OUT: profile_out/)
set -u
TAG=${1:-r02}
shift || true
cd "$(dirname "$0")/.."
REPO=$PWD
OUT=${PROFILE_OUT:-$REPO/profile_out}
export TMPDIR=/tmp
mkdir -p "$OUT/prof_$TAG"
( cd /tmp && rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_$TAG" -o trace -- python3 "$REPO/bench.py" --full --steps 3 --warmup 1 --resident-steps 5 --no-cpu-baseline --no-dense --no-bwa "$@" ) > "$OUT/prof_$TAG/bench_stdout.log" 2>&1
find "$OUT/prof_$TAG" -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} "$OUT/prof_${TAG}_kernel_stats.csv"
rm -f "$OUT/prof_$TAG"/*.db "$OUT/prof_$TAG"/*kernel_trace.csv
tail -c 400 "$OUT/prof_$TAG/bench_stdout.log"
head -30 "$OUT/prof_${TAG}_kernel_stats.csv"
