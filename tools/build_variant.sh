#!/bin/bash
# Build a variant of libmacm_hip.so with extra compile flags for A/B timing (tools/ab.sh):
#   tools/build_variant.sh NAME [-DFLAG ...]   ->  abv/NAME.so  (abv/ is git-ignored and ships with gpurun;
#   ab/ holds old variants and does not ship: .gpurunignore)
set -eu
cd "$(dirname "$0")/.."
NAME=$1; shift
mkdir -p abv/build_$NAME
PIDS=()
for src in gym-macm_amd/csrc/*.hip; do  # every unit, as tools/isa_snapshot.sh
  f=$(basename "$src" .hip)
  X=""; { [ $f = flock_rollout_w64 ] || [ $f = flock_rollout_ar_w64 ]; } && X="-mllvm -disable-machine-licm"  # as the Makefile
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize -Wall -Wno-unused-result $X "$@" \
    -c -o abv/build_$NAME/$f.o "$src" &
  PIDS+=($!)
done
for p in "${PIDS[@]}"; do wait "$p" || { echo "compile failed: abv/$NAME.so not built" >&2; rm -rf abv/build_$NAME; exit 1; }; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o abv/$NAME.so abv/build_$NAME/*.o
rm -rf abv/build_$NAME
echo "built abv/$NAME.so"
