#!/bin/bash
# Build the library of another commit next to the real one, for same-box A/B runs:
#   tools/build_prev.sh [rev = HEAD]  ->  tools/abl/prev.so ; run anything against it with FH_LIB_PATH=...
# (sources of that revision are checked out to a temporary directory and built by that revision's own build.py, so
# every file gets the flags it had there -- the per-source ones included; the working tree is not touched)
set -e
cd "$(dirname "$0")/.."
rev=${1:-HEAD}
d=$(mktemp -d); trap 'rm -rf $d' EXIT; mkdir -p tools/abl
git archive $rev flowhigh_amd/build.py flowhigh_amd/csrc include | tar -x -C $d
python3 $d/flowhigh_amd/build.py --force > $d/build.log 2>&1 || { tail -20 $d/build.log; exit 1; }
cp $d/flowhigh_amd/lib/libflowhigh_hip.so tools/abl/prev.so
echo tools/abl/prev.so "($rev)"
