#!/bin/bash
# Dirty-bytes-at-a-boundary probe (repo root): bash profiles/tools/dirty_boundary.sh [OUT_DIR]
# Builds profiles/tools/dirty_boundary.bin when it is missing (an ignored build product) and runs it at two spin lengths.
set -o pipefail
REPO=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${1:-$REPO/profiles/tools/dirty_boundary_out}
BIN=$REPO/profiles/tools/dirty_boundary.bin
mkdir -p "$OUT"
[ -x "$BIN" ] || hipcc --offload-arch=gfx950 -O3 -o "$BIN" "$REPO/profiles/tools/dirty_boundary.hip" || exit 1
timeout -k 10 120 "$BIN" 10 300 | tee "$OUT/dirty_boundary_spin10.txt" &&
timeout -k 10 120 "$BIN" 4 300 | tee "$OUT/dirty_boundary_spin4.txt"
