#!/bin/bash
# Build libe4t_hip.so for gfx950 (cross-compiles without a GPU).  Usage: csrc/build.sh
set -e
cd "$(dirname "$0")"
OUT=../e4t/libe4t_hip.so
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=fast -Wno-unused-result"
SRCS="core gemm attention norm wo elementwise image comm tome freeu"
mkdir -p obj
pids=()
for f in $SRCS; do
  if [ ! -f obj/$f.o ] || [ $f.hip -nt obj/$f.o ] || [ common.h -nt obj/$f.o ] || { [ $f = elementwise ] && { [ adamw_kernel.inc -nt obj/$f.o ] || [ adamw_rank_kernel.inc -nt obj/$f.o ]; }; } || { [ $f = gemm ] && { [ gemm_common.h -nt obj/$f.o ] || [ gemm_dma_kernel.inc -nt obj/$f.o ] || [ gemm_pq_kernel.inc -nt obj/$f.o ]; }; } || [ ../../include/e4t_hip.h -nt obj/$f.o ]; then
    EXTRA=""
    [ $f = image ] && EXTRA="-ffp-contract=off"      # byte-exact INTER_AREA: float ops must not be fused (see image.hip)
    [ $f = attention ] && EXTRA="-fno-slp-vectorize" # packing is chosen per kernel family in the source (attention.hip: PK_REG / PK_DMA); the SLP vectorizer's own costs the dh-40 backward 30 us
    hipcc $FLAGS $EXTRA -c $f.hip -o obj/$f.o &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p; done
hipcc --offload-arch=gfx950 -shared -fPIC $(printf 'obj/%s.o ' $SRCS) -ldl -o $OUT      # (the listed sources only: obj/ may hold objects of sources since removed)
echo "built $OUT"
