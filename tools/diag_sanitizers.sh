#!/bin/sh
# The staged diagnostics' entry points under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU: the library's HOST code
# is built with the sanitizers (device code as usual) and linked into a stand-alone program with its own main
# (tools/harness/diag_args_harness.c), which runs without a device.  Nothing here is loaded into Python.
#   sh tools/diag_sanitizers.sh [build dir, default /tmp/mcf_diag_asan]
set -e
cd "$(dirname "$0")/.."
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
OUT=${1:-/tmp/mcf_diag_asan}
SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
FLAGS="-O1 -g -std=c++17 -fPIC --offload-arch=gfx950 -mllvm -disable-machine-licm -Wno-unused-value -Wno-pass-failed"
mkdir -p "$OUT"
S=microclimf_amd/csrc
for u in mcf_kernels mcf_api mcf_terrain mcf_snow mcf_snowrun; do
    $HIPCC $FLAGS $SAN -c -o "$OUT/$u.o" $S/$u.hip &
done
$HIPCC $FLAGS $SAN -c -o "$OUT/mcf_hydro_dev.o" $S/mcf_hydro.hip &
$HIPCC $FLAGS $SAN -ffp-contract=off -c -o "$OUT/mcf_pointbatch.o" $S/mcf_pointbatch.hip &
$HIPCC $FLAGS $SAN -ffp-contract=off -c -o "$OUT/mcf_vegprep_dev.o" $S/mcf_vegprep.hip &
for u in mcf_pointmodel mcf_hydro mcf_vegprep; do
    $HIPCC -O1 -g -std=c++17 -fPIC -ffp-contract=off -fsanitize=address,undefined -fno-omit-frame-pointer -x c++ -c -o "$OUT/$u.o" $S/$u.cpp &
done
wait
$HIPCC -O1 -g -fsanitize=address,undefined -Iinclude -x c -c -o "$OUT/harness.o" tools/harness/diag_args_harness.c
$HIPCC --offload-arch=gfx950 -fsanitize=address,undefined -o "$OUT/diag_args" "$OUT"/*.o -lz -ldl -lm
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$OUT/diag_args"
