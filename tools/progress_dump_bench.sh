#!/bin/bash
# tools/progress_dump_bench.py, every step under a time limit of its own and chained with &&: a step that faults, hangs or
# runs over ends the script, nothing further is started on the GPU.  -> profiles/progress_dump_bench.json
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${1:-profiles/progress_dump_bench.json}
WORK=$(mktemp -d)
trap 'rm -rf "$WORK"' EXIT
export TMPDIR="$WORK"                  # the steps' own temporary logdirs go under it as well
B="python tools/progress_dump_bench.py"
timeout -k 10 300 $B dataset --dir "$WORK/data" --out "$WORK/0.json" > /dev/null && echo "dataset written" &&
timeout -k 10 240 $B dump --dir "$WORK/data" --out "$WORK/1.json" > /dev/null && echo "dump timed" &&
timeout -k 10 360 $B steps --dir "$WORK/data" --out "$WORK/2.json" > /dev/null &&
$B merge "$WORK"/[0-2].json --out "$OUT"
