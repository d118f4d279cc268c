#!/bin/bash
# tools/sanitize_dose.sh -- the CPU form of the dose rule (host/Dose.cpp)
# under AddressSanitizer + UBSan, as a stand-alone program (tools/dose_selftest.cpp): no Python, no GPU.
# Prints the program's verdict and the number of sanitizer reports (expected: 0 and 0).
set -eu
ROOT=$(cd "$(dirname "$0")/.." && pwd)
W=$(mktemp -d)
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -ffp-contract=off -Wall -Wextra \
    -I "$ROOT/include" -I "$ROOT/ray_tracing_octrees_amd/host" \
    "$ROOT/ray_tracing_octrees_amd/host/Dose.cpp" \
    "$ROOT/tools/dose_selftest.cpp" -o "$W/dose_selftest"
rc=0
UBSAN_OPTIONS=print_stacktrace=1 "$W/dose_selftest" > "$W/log" 2>&1 || rc=$?
tail -5 "$W/log"
echo "exit code: $rc"
echo "UBSan reports: $(grep -c 'runtime error' "$W/log" || true)"
echo "ASan reports: $(grep -c 'ERROR: AddressSanitizer' "$W/log" || true)"
rm -rf "$W"
exit $rc
