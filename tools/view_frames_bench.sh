#!/bin/bash
# tools/view_frames_bench.py, every step under a time limit of its own and chained with &&: a step that faults, hangs or
# runs over ends the script, nothing further is started on the GPU.  -> profiles/view_frames_bench.json
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${1:-profiles/view_frames_bench.json}
WORK=$(mktemp -d)
trap 'rm -rf "$WORK"' EXIT
B="python tools/view_frames_bench.py"
timeout -k 10 240 $B dataset --dir "$WORK/data" --out "$WORK/0.json" > /dev/null &&
timeout -k 10 180 $B builder --dir "$WORK/data" --out "$WORK/1.json" > /dev/null &&
$B merge "$WORK"/[0-1].json --out "$OUT"
