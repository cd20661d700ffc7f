#!/bin/bash
# API-level launch trace (test infrastructure): every unit of csrc/build.sh compiled for the host alone, unchanged, and
# linked with a program that defines the few HIP runtime symbols the library calls (api_trace.hip), so that each C ABI
# call records its launches instead of reaching a GPU.  No GPU code, no GPU.
# SMX_TRACE_CSRC / SMX_TRACE_OUT: another source directory / program name (re-recording expected.txt: DESIGN.md section 2, Kernels).
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
CSRC=${SMX_TRACE_CSRC:-../../tensor-cuda-fft-_amd/csrc}
OUT=${SMX_TRACE_OUT:-api_trace}
UNITS="smx_decim smx_fourstep smx_fourstep2 smx_conv1 smx_direct smx_block smx_enh smx_time smx_ema smx_stream smx_byte smx_match smx_sst smx_api"
stale=0
[ -f "$OUT" ] || stale=1
for f in api_trace.hip build.sh ../../include/smx.h "$CSRC"/*.h "$CSRC"/*.hip; do
  [ "$f" -nt "$OUT" ] && stale=1
done
if [ $stale = 1 ]; then
  OBJ=$(mktemp -d)
  trap 'rm -rf "$OBJ"' EXIT
  FLAGS="--cuda-host-only -O1 -std=c++17 -I $CSRC -I ../../include"
  PIDS=""
  for u in $UNITS; do                     # fourteen units + the program: fifteen jobs
    $HIPCC $FLAGS -c "$CSRC/$u.hip" -o "$OBJ/$u.o" &
    PIDS="$PIDS $!"
  done
  $HIPCC $FLAGS -c api_trace.hip -o "$OBJ/main.o"
  for p in $PIDS; do wait $p; done
  # a host-only object still refers to its (absent) code object: the symbols resolve to 0 (nothing reads them:
  # api_trace.hip defines the registration entry points itself)
  DEFS=""
  for sym in $(nm -u "$OBJ"/*.o | grep -o '__hip_fatbin_[0-9a-f]*' | sort -u); do DEFS="$DEFS -Wl,--defsym=$sym=0"; done
  $HIPCC $DEFS -o "$OUT" "$OBJ"/*.o
fi
echo "built $(pwd)/$OUT"
