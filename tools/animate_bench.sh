#!/bin/bash
# tools/animate_bench.py, every step under a time limit of its own and chained with &&: a step that faults, hangs or
# runs over ends the script, nothing further is started on the GPU.  -> profiles/animate_bench.json
#   bash tools/animate_bench.sh [OUT.json [PARENT_TREE]]
# PARENT_TREE: a checkout of the parent commit with its library built; the movement way then runs that tree's run.py.
# Without it the movement way runs this tree's, and the JSON says so.
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${1:-profiles/animate_bench.json}
TREE=${2:+--tree $(cd "$2" && pwd)}
WORK=$(mktemp -d)
trap 'rm -rf "$WORK"' EXIT
B="python tools/animate_bench.py"
R="$B render --data $WORK/data --dir $WORK"
timeout -k 10 240 $B kernel --out "$WORK/0.json" > /dev/null &&
timeout -k 10 240 $B dataset --data "$WORK/data" --out "$WORK/1.json" > /dev/null &&
timeout -k 10 240 $R --way movement $TREE --out "$WORK/2.json" &&
timeout -k 10 240 $R --way animate --out "$WORK/3.json" &&
timeout -k 10 240 $R --way animate_skeleton --out "$WORK/4.json" &&
timeout -k 10 240 $R --way movement $TREE --out "$WORK/5.json" &&
timeout -k 10 240 $R --way animate --out "$WORK/6.json" &&
timeout -k 10 240 $R --way animate_skeleton --out "$WORK/7.json" &&
timeout -k 10 240 $R --way movement $TREE --out "$WORK/8.json" &&
timeout -k 10 240 $R --way animate --out "$WORK/9.json" &&
timeout -k 10 240 $R --way animate_skeleton --out "$WORK/10.json" &&
$B merge "$WORK"/[0-9].json "$WORK"/10.json --out "$OUT"
