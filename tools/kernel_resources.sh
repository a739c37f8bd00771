#!/bin/bash
# usage: tools/kernel_resources.sh <file.hip> -> per-kernel VGPR / AGPR / spill / occupancy / LDS summary (gfx950)
# Compiled as the product compiles it: the flags the file has in vcap/build.py's FILE_FLAGS (keyed by file
# name, so a copy of another revision's file under its own name gets them too).
root=$(cd "$(dirname "$0")/.." && pwd)
out=$root/gpurun_out/scratch; mkdir -p $out
extra=$(cd $root/video-caption-algorithm_amd && python3 -c "
import sys
from vcap.build import FILE_FLAGS
print(' '.join(FILE_FLAGS.get(sys.argv[1], [])))" "$(basename "$1")") || exit 1
/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -I$root/video-caption-algorithm_amd/csrc -I$root/include $extra \
  -c "$1" -Rpass-analysis=kernel-resource-usage -o $out/res.o 2>&1 | python3 -c "
import sys, re
cur = None
for line in sys.stdin:
    m = re.search(r'Function Name: (\S+)', line)
    if m:
        cur = m.group(1); print(); print(cur[:70], end=' ')
    m = re.search(r'(VGPRs|AGPRs|VGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)', line)
    if m and cur:
        print(m.group(1).split()[0] + ('S' if 'Spill' in m.group(1) else '') + '=' + m.group(2), end=' ')
print()
"
