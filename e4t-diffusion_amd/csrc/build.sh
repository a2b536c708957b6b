#!/bin/bash
# Build libe4t_hip.so for gfx950 (cross-compiles without a GPU).  Usage: csrc/build.sh
set -e
cd "$(dirname "$0")"
. ./units.sh      # UNITS, UNIT_FLAGS, unit_extra_flags, unit_extra_deps
OUT=../e4t/libe4t_hip.so
mkdir -p obj
pids=()
for f in $UNITS; do
  stale=0
  for d in $f.hip common.h ../../include/e4t_hip.h $(unit_extra_deps $f); do
    if [ ! -f obj/$f.o ] || [ $d -nt obj/$f.o ]; then stale=1; fi
  done
  if [ $stale = 1 ]; then
    hipcc $UNIT_FLAGS $(unit_extra_flags $f) -c $f.hip -o obj/$f.o &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p; done
hipcc --offload-arch=gfx950 -shared -fPIC $(printf 'obj/%s.o ' $UNITS) -ldl -o $OUT      # (the listed sources only: obj/ may hold objects of sources since removed)
echo "built $OUT"
