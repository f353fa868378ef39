#!/usr/bin/env bash
# rocprofv3 kernel trace + stats of the bench's rotating leg (`bench.py --full --no-cpu-baseline --no-extras`).
# usage: bash scripts/gpu_profile.sh <tag> [bench args...]   -> $NFP_PROFILE_DIR/prof_<tag>/ (default profile_out/)
set -u
tag=${1:-run}; shift || true
cd "$(dirname "$0")/.."
out=${NFP_PROFILE_DIR:-profile_out}/prof_$tag
mkdir -p $out
export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $out -o trace -- \
  python3 bench.py --full --no-cpu-baseline --no-extras "$@" > $out/bench.log 2>&1
rc=$?
echo "rocprof rc=$rc"; tail -n 3 $out/bench.log
find $out -name '*stats*' | head
f=$(find $out -name '*kernel_stats.csv' | head -1)
[ -n "$f" ] && head -20 "$f"
exit $rc
