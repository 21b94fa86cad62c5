#!/bin/bash
# tools/mesh_normal_bench.py, every step under a time limit of its own and chained with &&, one process at a time: a step that
# faults, hangs or runs over ends the script, nothing further is started on the GPU.  -> profiles/mesh_normal_bench.json
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${1:-profiles/mesh_normal_bench.json}
WORK=$(mktemp -d)
trap 'rm -rf "$WORK"' EXIT
B="python tools/mesh_normal_bench.py"
timeout -k 10 300 $B device --state "$WORK/state.npz" --out "$WORK/0.json" > /dev/null &&
timeout -k 10 240 $B numpy --state "$WORK/state.npz" --out "$WORK/1.json" > /dev/null &&
$B merge "$WORK"/[0-1].json --out "$OUT"
