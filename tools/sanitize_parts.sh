#!/bin/bash
# tools/sanitize_parts.sh -- the CPU form of the part-segmentation rule (host/Parts.cpp over host/Distance.cpp's transform, checked
# at ratio 0 against host/Components.cpp) under AddressSanitizer + UBSan, as a stand-alone program (tools/parts_selftest.cpp): no
# Python, no GPU.  Prints the program's verdict and the number of sanitizer reports (expected: 0 and 0).
set -eu
ROOT=$(cd "$(dirname "$0")/.." && pwd)
W=$(mktemp -d)
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -ffp-contract=off -Wall -Wextra \
    -I "$ROOT/include" -I "$ROOT/ray_tracing_octrees_amd/host" \
    "$ROOT/ray_tracing_octrees_amd/host/Distance.cpp" "$ROOT/ray_tracing_octrees_amd/host/Components.cpp" \
    "$ROOT/ray_tracing_octrees_amd/host/Parts.cpp" "$ROOT/tools/parts_selftest.cpp" -o "$W/parts_selftest"
rc=0
UBSAN_OPTIONS=print_stacktrace=1 "$W/parts_selftest" > "$W/log" 2>&1 || rc=$?
tail -5 "$W/log"
echo "exit code: $rc"
echo "UBSan reports: $(grep -c 'runtime error' "$W/log" || true)"
echo "ASan reports: $(grep -c 'ERROR: AddressSanitizer' "$W/log" || true)"
rm -rf "$W"
exit $rc
