#!/bin/bash
# tools/resize_bench.py, every step under a time limit of its own and chained with &&: a step that faults, hangs or
# runs over ends the script, nothing further is started on the GPU.  -> profiles/resize_bench.json
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${1:-profiles/resize_bench.json}
WORK=$(mktemp -d)
trap 'rm -rf "$WORK"' EXIT
B="python tools/resize_bench.py"
timeout -k 10 300 $B dataset --dir "$WORK/data" --out "$WORK/0.json" > /dev/null &&
timeout -k 10 120 $B kernel --dir "$WORK/data" --out "$WORK/1.json" > /dev/null &&
timeout -k 10 300 $B step --dir "$WORK/data" --out "$WORK/2.json" > /dev/null &&
$B merge "$WORK"/[0-2].json --out "$OUT"
