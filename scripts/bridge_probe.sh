#!/bin/bash
# bridge_probe.py timed, then the kernel trace of the same command in a run of its own (profiles/bridge_tick.md).
# usage: scripts/bridge_probe.sh [output directory]
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${1:-build/bridge_probe}
mkdir -p "$OUT"
timeout -k 10 240 python scripts/bridge_probe.py 2>&1 | tee "$OUT/bridge_probe.jsonl" &&
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace" -o bridge -- python scripts/bridge_probe.py --trace > "$OUT/trace.log" 2>&1 &&
cat "$OUT"/trace/*kernel_stats.csv | head -20
