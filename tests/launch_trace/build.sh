#!/bin/bash
# Launch-selection trace (test infrastructure): the launchers of the transform families compiled for the host alone
# with SMX_LAUNCH_TRACE, so that SMX_LAUNCH records the instance and grid instead of launching.  No GPU code, no GPU.
# SMX_TRACE_CSRC / SMX_TRACE_OUT: another source directory / program name (re-recording expected.txt: DESIGN.md section 2, Kernels).
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
CSRC=${SMX_TRACE_CSRC:-../../tensor-cuda-fft-_amd/csrc}
OUT=${SMX_TRACE_OUT:-launch_trace}
UNITS="smx_decim smx_conv1 smx_fourstep smx_fourstep2"
stale=0
[ -f "$OUT" ] || stale=1
for f in launch_trace.hip build.sh "$CSRC"/*.h "$CSRC"/smx_decim.hip "$CSRC"/smx_conv1.hip "$CSRC"/smx_fourstep.hip "$CSRC"/smx_fourstep2.hip; do
  [ "$f" -nt "$OUT" ] && stale=1
done
if [ $stale = 1 ]; then
  OBJ=$(mktemp -d)
  trap 'rm -rf "$OBJ"' EXIT
  PIDS=""
  for u in $UNITS; do
    $HIPCC --cuda-host-only -DSMX_LAUNCH_TRACE -O1 -std=c++17 -Wno-unused-result -I "$CSRC" -c "$CSRC/$u.hip" -o "$OBJ/$u.o" &
    PIDS="$PIDS $!"
  done
  $HIPCC --cuda-host-only -DSMX_LAUNCH_TRACE -O1 -std=c++17 -I "$CSRC" -c launch_trace.hip -o "$OBJ/main.o"
  for p in $PIDS; do wait $p; done
  # a host-only object still refers to its (absent) code object: the symbols resolve to 0, and the program registers
  # nothing with the HIP runtime (launch_trace.hip defines the registration entry points itself; a unit that gains a
  # __device__ or __constant__ variable will need __hipRegisterVar there as well)
  DEFS=""
  for sym in $(nm -u "$OBJ"/*.o | grep -o '__hip_fatbin_[0-9a-f]*' | sort -u); do DEFS="$DEFS -Wl,--defsym=$sym=0"; done
  $HIPCC $DEFS -o "$OUT" "$OBJ"/*.o
fi
echo "built $(pwd)/$OUT"
