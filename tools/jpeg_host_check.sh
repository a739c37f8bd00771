#!/bin/bash
# The JPEG host stage (csrc/jpeg.hip: parse + entropy decode) under AddressSanitizer and UBSan on the CPU:
# builds tools/jpeg_host_check.cpp with jpeg.hip as one stand-alone program (host code instrumented, no
# LD_PRELOAD, no device call) and runs it over the files of the JPEG sweep's case table.
#   tools/jpeg_host_check.sh [CASE_DIR]               CASE_DIR: output of `python tests/jpeg_cases.py --dump DIR`
#                                                     (dumped to a temporary directory when not given)
#   JPEG_HIP=path/to/jpeg.hip HEADER_ONLY=1 tools/jpeg_host_check.sh [CASE_DIR]
#                                                     another jpeg.hip, vcap_jpeg_header alone (a source from
#                                                     before the host stage was split off)
# Exit status 0: every call returned 0, VCAP_E_ARG or VCAP_E_UNSUPPORTED and no sanitizer reported.
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
CSRC="$ROOT/video-caption-algorithm_amd/csrc"
HIPCC="${HIPCC:-$(command -v hipcc || echo /opt/rocm/bin/hipcc)}"
WORK="$(mktemp -d)"
trap 'rm -rf "$WORK"' EXIT
CASES="${1:-}"
if [ -z "$CASES" ]; then
  CASES="$WORK/cases"
  python "$ROOT/tests/jpeg_cases.py" --dump "$CASES"
fi
DEFS=()
[ -n "${HEADER_ONLY:-}" ] && DEFS+=(-DJPEG_HOST_CHECK_HEADER_ONLY)
# host code only is instrumented (-Xarch_host); the sanitizer runtimes come in at the link of the two objects
for src in "$ROOT/tools/jpeg_host_check.cpp" "${JPEG_HIP:-$CSRC/jpeg.hip}"; do
  "$HIPCC" --offload-arch=gfx950 -std=c++17 -O1 -g -fno-omit-frame-pointer -Xarch_host -fsanitize=address,undefined \
    -Xarch_host -fno-sanitize-recover=undefined "${DEFS[@]}" -I"$CSRC" -I"$ROOT/include" -x hip -c "$src" \
    -o "$WORK/$(basename "$src").o"
done
"$HIPCC" -fsanitize=address,undefined "$WORK"/*.o -o "$WORK/jpeg_host_check"
# the HIP runtime the program links keeps process-lifetime allocations: leak checking would only report those
ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=print_stacktrace=1 "$WORK/jpeg_host_check" "$CASES"/*.jpg
