#!/bin/bash
# Builds an EXPERIMENT twin of the library (not the product) whose row expansion counts, per chunk launch and XCD, the items its workgroups
# take from their own zone and from other zones (minhash_kernels.hip ES_STEAL_COUNT; read by tools/expand_steals.py).
#   tools/experiments/build_steal_count.sh   -> tools/experiments/lib/libsteals.so
set -e
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
make -s -C "$ROOT/dynaalign_amd/csrc" BUILD=build_steals OUT="$ROOT/tools/experiments/lib/libsteals.so" \
  CXXFLAGS="-O3 -std=c++17 -fPIC -fwrapv --offload-arch=gfx950 -Wall -Wno-unused-function -DES_STEAL_COUNT"
echo "built $ROOT/tools/experiments/lib/libsteals.so"
