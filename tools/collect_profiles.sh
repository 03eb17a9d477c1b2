#!/bin/bash
# Run ON THE GPU BOX: rocprofv3 kernel-trace stats + HBM PMC passes of the bench command.
#   tools/collect_profiles.sh r01 [extra bench.py arguments]
# Writes raw output under gpurun_out/prof_<tag>/ ; tools/profile_summary.py turns it into profiles/<tag>_*.
# Every GPU step runs under its own time limit and the steps are chained: the script stops at the first failure.
set -u
TAG=${1:-r01}
shift || true
EXTRA="$*"                         # extra bench.py arguments, e.g. --resolution 512 --batch 32, --model recnext_a3
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$ROOT/gpurun_out/prof_$TAG
STEP_S=${PROFILE_STEP_SECONDS:-1200}      # time limit of one profiled bench run
SUMMARY_DIR=$(dirname "$OUT")/profiles_$TAG
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
cd "$ROOT"
CMD="python3 bench.py --steps 20 --warmup 10 --no-cpu-baseline $EXTRA"
# counters in their own passes (FETCH_SIZE and WRITE_SIZE do not fit one pass on gfx950)
timeout -k 10 "$STEP_S" rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/kt" -- $CMD > "$OUT/kt_bench.log" 2>&1 &&
timeout -k 10 "$STEP_S" rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/pmc_fetch" -- $CMD > "$OUT/pmc_fetch.log" 2>&1 &&
timeout -k 10 "$STEP_S" rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$OUT/pmc_write" -- $CMD > "$OUT/pmc_write.log" 2>&1 &&
timeout -k 10 300 python3 tools/profile_summary.py "$TAG" "$OUT" "$SUMMARY_DIR"
rc=$?
ls -la "$SUMMARY_DIR" 2>/dev/null
rm -rf "$OUT/kt" "$OUT/pmc_fetch" "$OUT/pmc_write"      # the raw traces are tens of MB per configuration: gpurun copies back at most 64 MiB
exit $rc
