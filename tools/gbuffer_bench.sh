#!/bin/bash
# tools/gbuffer_bench.py, every step under a time limit of its own and chained with &&: a step that faults, hangs or
# runs over ends the script, nothing further is started on the GPU.  -> profiles/gbuffer_bench.json
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${1:-profiles/gbuffer_bench.json}
WORK=$(mktemp -d)
trap 'rm -rf "$WORK"' EXIT
B="python tools/gbuffer_bench.py"
timeout -k 10 240 $B kernels --out "$WORK/0.json" > /dev/null &&
timeout -k 10 150 $B movement --dir "$WORK" --geometry 0 --out "$WORK/1.json" > /dev/null &&
timeout -k 10 150 $B movement --dir "$WORK" --geometry 1 --min-alpha 0.05 --out "$WORK/2.json" > /dev/null &&
timeout -k 10 150 $B movement --dir "$WORK" --geometry 0 --out "$WORK/3.json" > /dev/null &&
timeout -k 10 150 $B movement --dir "$WORK" --geometry 1 --min-alpha 0.05 --out "$WORK/4.json" > /dev/null &&
timeout -k 10 150 $B movement --dir "$WORK" --geometry 0 --out "$WORK/5.json" > /dev/null &&
timeout -k 10 150 $B movement --dir "$WORK" --geometry 1 --min-alpha 0.05 --out "$WORK/6.json" > /dev/null &&
$B merge "$WORK"/[0-6].json --out "$OUT"
