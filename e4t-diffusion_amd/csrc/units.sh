# The translation units of libe4t_hip.so and how each is compiled: the one list that csrc/build.sh and the tools that compile or
# link the units themselves (tools/build_variant.sh, check_isa.sh, pp_trace.sh, dma_trace.sh) source.  UNIT.hip -> obj/UNIT.o.
UNITS="core gemm attention norm wo elementwise optim sampler objective image comm tome freeu"
UNIT_FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=fast -Wno-unused-result"      # every unit
# flags of one unit on top of UNIT_FLAGS
unit_extra_flags() {
  case $1 in
    image) echo "-ffp-contract=off" ;;          # byte-exact INTER_AREA: float ops must not be fused (see image.hip)
    attention) echo "-fno-slp-vectorize" ;;     # packing is chosen per kernel family in the source (attention.hip: PK_REG / PK_DMA); the SLP vectorizer's own costs the dh-40 backward 30 us
  esac
}
# what a unit includes besides common.h and include/e4t_hip.h
unit_extra_deps() {
  case $1 in
    gemm) echo "gemm_common.h gemm_dma_kernel.inc gemm_pq_kernel.inc" ;;
    optim) echo "adamw_kernel.inc adamw_rank_kernel.inc" ;;
  esac
}
