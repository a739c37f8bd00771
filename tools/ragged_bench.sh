#!/bin/bash
# usage: tools/ragged_bench.sh prepare   (CPU box) export the parent commit to abl/parent and build its library there
#        tools/ragged_bench.sh run [out] (GPU box) tools/ragged_bench.py against abl/parent -> out (default
#                                         profiles/ragged_prompts.txt)
set -e
root=$(cd "$(dirname "$0")/.." && pwd)
case "$1" in
  prepare)
    rm -rf $root/abl/parent; mkdir -p $root/abl/parent
    git -C $root archive HEAD | tar -x -C $root/abl/parent
    mkdir -p $root/abl/parent/video-caption-algorithm_amd/vcap/_lib
    $root/tools/build_ref_lib.sh HEAD $root/abl/parent/video-caption-algorithm_amd/vcap/_lib/libvcap_hip.so ;;
  run)
    python3 $root/tools/ragged_bench.py $root/abl/parent --out ${2:-$root/profiles/ragged_prompts.txt} ;;
  *) echo "usage: $0 prepare | run [out]"; exit 2 ;;
esac
