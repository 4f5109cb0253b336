#!/bin/bash
# Builds the EXPERIMENT twin of the library (not the product): libdynaalign_hip.so + round 4's generated NW rows
# (tools/gen_nw_asm.py -> nw_rows_p12 / p20.inc) behind DYNAALIGN_NW_ASM=1.
#   tools/experiments/build.sh          -> tools/experiments/lib/libdynaalign_hip.so
#   DYNAALIGN_LIB=tools/experiments/lib/libdynaalign_hip.so python tools/nw_time.py ...      (dynaalign_amd/_capi.py honours DYNAALIGN_LIB)
set -e
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
for n in 12 20; do NWASM_NMAX=$n python3 "$ROOT/tools/gen_nw_asm.py" "$ROOT/tools/experiments/nw_rows_p$n.inc" > /dev/null; done
make -s -C "$ROOT/dynaalign_amd/csrc" BUILD=build_experiments OUT="$ROOT/tools/experiments/lib/libdynaalign_hip.so" \
  CXXFLAGS="-O3 -std=c++17 -fPIC -fwrapv --offload-arch=gfx950 -Wall -Wno-unused-function -DDA_K2_EXPERIMENTS -I. -I$ROOT/tools/experiments"
echo "built $ROOT/tools/experiments/lib/libdynaalign_hip.so"
