// MFMA GEMM / implicit-GEMM 3x3 convolution for gfx950 (CDNA4).
//
//   C[M,N] = epilogue( alpha * A[M,K] . B[N,K]^T )          ("NT": both operands K-contiguous)
//
// A is either a dense row-major matrix (optionally split over two sources along K, which is how
// torch.cat([h, skip], 1) feeds a 1x1 shortcut conv without materialising the concat), or the
// im2col view of an NHWC activation (3x3 taps, pad 1; stride 1 / stride 2 / fused nearest-x2
// upsample / stride-2 transposed for dgrad) gathered on the fly — no im2col buffer ever exists.
//
// Layout: activations are NHWC bf16, i.e. a (B*H*W, C) row-major matrix, everywhere in this
// library.  Conv weights are pre-laid-out as [Cout][ky][kx][Cin] (K = 9*Cin contiguous).
//
// Kernel: 4 waves (256 threads) per workgroup, block tile BM x BN x 64, register-staged
// global->LDS copy with the next tile's global loads in flight under the current tile's MFMAs,
// LDS rows padded to 72 bf16 (144 B) so that ds_read_b128 fragment reads are bank-conflict free
// (16 distinct 16-B slots per 16-lane group), v_mfma_f32_32x32x16_bf16 with fp32 accumulation.
// Fused epilogue: alpha, per-column bias, per-(batch,column) bias (the ResBlock time-embedding
// add), residual add (bf16 or fp32), exact-erf GELU, accumulate-into-C, bf16 or fp32 store.
// Optional split-K (grid.z) through an fp32 workspace + a deterministic reduce/epilogue kernel
// (used for the K=11520..23040, M=1024 convs at the 8x8 level and for weight-gradient GEMMs whose
// reduction runs over B*H*W).
//
// Host half (end of this file): one table, kVariants, has a row per kernel variant — tile code, tile shape, capabilities, entry points
// and their symbol text.  plan_gemm() (hint -> automatic choice -> capability fallback -> split-K) picks a row, launch_gemm() launches
// the row's entry and logs the row's text; e4t_gemm_plan / e4t_conv3x3_plan export the same plan.
// Operand addressing the kernels share (batch entry, output pixel, LDS swizzle / fragment offsets, strip geometry): gemm_common.h.
//
// Reference call sites this replaces: every F.linear / nn.Linear / nn.Conv2d on the hot path —
// e4t/models/cross_attention.py:506,516,518,534 ; e4t/models/attention.py:376,419-430 ;
// e4t/models/transformer_2d.py:153,205,258-261 ; [3P diffusers] ResnetBlock2D/Downsample2D/Upsample2D
// constructed at e4t/models/unet_2d_blocks.py:481,760,804,881,1732,1774,1855,1872 ;
// e4t/models/unet_2d_condition.py:106-108,285-287 ; [3P open_clip] ViT linears (e4t/encoder.py:154).
#include "gemm_common.h"

namespace {


// MODE 0: dense A.  MODE 1: implicit 3x3 conv over NHWC A.
template <int BM, int BN, int WGM, int WGN, int MODE>
__global__ __launch_bounds__(256) void gemm_kernel(GemmArgs p) {
  constexpr int WM = BM / WGM, WN = BN / WGN;  // per-wave tile
  constexpr int FM = WM / 32, FN = WN / 32;    // 32x32 MFMA fragments per wave
  constexpr int NA = BM * (BK / 8) / 256;      // 16-B chunks of A per thread per K-tile
  constexpr int NB = BN * (BK / 8) / 256;
  static_assert(WGM * WGN == 4, "4 waves per workgroup");
  static_assert(NA >= 1 && NB >= 1, "tile too small");

  __shared__ __attribute__((aligned(16))) bf16_t smem[(BM + BN) * LDS_LD];
  bf16_t* const As = smem;
  bf16_t* const Bs = smem + BM * LDS_LD;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WGN, wn = wave % WGN;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;

  const KRange kr = batch_entry<BK>(p, (p.K + BK - 1) / BK);
  const int kt_begin = kr.begin, kt_end = kr.end;

  // ---- per-thread chunk ownership (fixed rows across the K loop) ----
  // chunk c = tid + i*256 : row = c >> 3, kc = c & 7  (8 lanes cover one 128-B row segment)
  int a_row[NA];
  long long a_base[NA];  // dense: row offset (elements) ; conv: packed (b, oy, ox)
  int a_oy[NA], a_ox[NA];
  bool a_ok[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int c = tid + i * 256;
    const int r = c >> 3;
    a_row[i] = r;
    const int gr = m0 + r;
    a_ok[i] = gr < p.M;
    if (MODE == 0) {
      a_base[i] = (long long)gr;
      a_oy[i] = a_ox[i] = 0;
    } else {
      out_pixel(p, gr, a_base[i], a_oy[i], a_ox[i]);
    }
  }
  const int kc8 = (tid & 7) * 8;  // this thread's k offset inside a tile (same for all its chunks)

  uint4 ra[NA], rb[NB];

  auto load_tile = [&](int kt) {
    const int k0 = kt * BK;
    const int k = k0 + kc8;
    if (MODE == 0) {
      const bf16_t* src = p.A;
      int ld = p.lda, kk = k;
      if (k0 >= p.K1) { src = p.A2; ld = p.lda2; kk = k - p.K1; }
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (a_ok[i] && k < p.K) v = *(const uint4*)(src + a_base[i] * ld + kk);
        ra[i] = v;
      }
    } else {
      const int tap = k0 / p.Cin;
      const int ci = k - tap * p.Cin;
      const int ky = tap / 3, kx = tap - ky * 3;
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        int iy, ix;
        bool ok = a_ok[i];      // written out: profiles/gemm_addressing_isa.txt
        if (p.mode == E4T_CONV_S1) {
          iy = a_oy[i] + ky - 1; ix = a_ox[i] + kx - 1;
          ok = ok && iy >= 0 && iy < p.Hin && ix >= 0 && ix < p.Win;
        } else if (p.mode == E4T_CONV_S2) {
          iy = 2 * a_oy[i] + ky - 1; ix = 2 * a_ox[i] + kx - 1;
          ok = ok && iy >= 0 && iy < p.Hin && ix >= 0 && ix < p.Win;
        } else if (p.mode == E4T_CONV_UP2) {  // logical input = nearest-x2 upsample of X
          iy = a_oy[i] + ky - 1; ix = a_ox[i] + kx - 1;
          ok = ok && iy >= 0 && iy < 2 * p.Hin && ix >= 0 && ix < 2 * p.Win;
          iy >>= 1; ix >>= 1;
        } else if (p.mode == E4T_CONV_S2A) {  // stride 2, pad (0,1,0,1): the VAE encoder's Downsample2D(padding=0)
          iy = 2 * a_oy[i] + ky; ix = 2 * a_ox[i] + kx;
          ok = ok && iy < p.Hin && ix < p.Win;
        } else {  // E4T_CONV_S2T: transposed stride-2 (dgrad of S2); X is the (smaller) output-grad map
          const int sy = a_oy[i] + ky - 1, sx = a_ox[i] + kx - 1;
          ok = ok && sy >= 0 && sx >= 0 && !(sy & 1) && !(sx & 1);
          iy = sy >> 1; ix = sx >> 1;
          ok = ok && iy < p.Hin && ix < p.Win;
        }
        uint4 v = make_uint4(0, 0, 0, 0);
        if (ok) v = *(const uint4*)(p.A + (a_base[i] + (long long)iy * p.Win + ix) * p.Cin + ci);
        ra[i] = v;
      }
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int r = (tid + i * 256) >> 3;
      const int gn = n0 + r;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (gn < p.N && k < p.K) v = *(const uint4*)(p.B + (size_t)gn * p.ldb + k);
      rb[i] = v;
    }
  };

  f32x16 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if (kt_begin < kt_end) load_tile(kt_begin);

  const int frow = lane & 31, fhi = lane >> 5;
  for (int kt = kt_begin; kt < kt_end; ++kt) {
#pragma unroll
    for (int i = 0; i < NA; ++i) *(uint4*)(As + a_row[i] * LDS_LD + kc8) = ra[i];
#pragma unroll
    for (int i = 0; i < NB; ++i) *(uint4*)(Bs + ((tid + i * 256) >> 3) * LDS_LD + kc8) = rb[i];
    __syncthreads();
    if (kt + 1 < kt_end) load_tile(kt + 1);
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      bf16x8 af[FM], bfr[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i)
        af[i] = *(const bf16x8*)(As + (wm * WM + i * 32 + frow) * LDS_LD + ks * 16 + fhi * 8);
#pragma unroll
      for (int j = 0; j < FN; ++j)
        bfr[j] = *(const bf16x8*)(Bs + (wn * WN + j * 32 + frow) * LDS_LD + ks * 16 + fhi * 8);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  write_tile<WM, WN, FM, FN, true>(p, acc, wave_stage<WM, WN>(smem, wave), lane, m0 + wm * WM, n0 + wn * WN);
}

// ------------------------------------------------------------------------------------------------
// LDS-DMA variant (the default): operand tiles go HBM -> LDS with global_load_lds_dwordx4, never
// through VGPRs or ds_write (the register-staged kernel above is LDS-write bound: 32 KB of
// ds_write_b128 per K-tile cost about as many LDS cycles as the tile's MFMAs take).
//   * one wave-instruction moves 8 rows x 128 B = 1 KiB, landing lane-linear in LDS, so tiles are
//     UNPADDED [rows][64] bf16; bank conflicts on the ds_read_b128 fragment reads are removed by an XOR
//     swizzle applied on the SOURCE side: LDS chunk slot p of row r holds logical 16-B chunk
//     p ^ ((r >> 1) & 7); fragment reads apply the same involution (16 rows distinct mod 16 -> 16
//     distinct 16-B slots per lane group);
//   * two LDS buffers, ONE barrier per K-tile: the DMA of tile t+1 is issued right after the barrier
//     that publishes tile t and flies under tile t's MFMAs;
//   * out-of-range rows / conv padding / K tail: the lane's source pointer is redirected to a 16-byte
//     zero word in global memory (DMA cannot synthesise zeros).
// ------------------------------------------------------------------------------------------------

#ifdef DMA_TRACE    // debug builds only (tools/dma_trace.sh): cycle stamps of wave 0 of every 8th workgroup
__device__ unsigned long long g_dma_trace[128 * 16];
#define DT(slot) do { if (dt_on) g_dma_trace[dt_wg * 16 + (slot)] = __builtin_readcyclecounter(); } while (0)
#else
#define DT(slot) do { } while (0)
#endif
// KT: K-tile width.  64 (128-byte rows, 8 rows per 1-KiB DMA piece) or 32 (64-byte rows, 16 rows per piece): the same LDS budget
// then holds twice the stages — 4 x 16 KiB instead of 2 x 32 KiB for the 128 x 128 tile, still two workgroups per CU — i.e. 3 K-tiles
// (48 KiB) instead of 1 (32 KiB) in flight per workgroup.  The cycle-stamp trace (tools/dma_trace.sh) shows the K loop of every
// shape waiting ~1700-2500 cycles per 64-wide tile for a DMA issued one iteration earlier against ~500 cycles of MFMA work.
template <int BM, int BN, int WGM, int WGN, int MODE, int NSTAGE, bool GENERAL = false, int KT = 64>
// (second argument = waves per SIMD the register allocation must leave room for: the 2-stage 128 x 160 tile runs TWO 4-wave workgroups per CU — at 260
// registers instead of 256 it ran one, 40 % slower: M16384 N640 K640 22.8 -> 31.9 us, round 6)
__global__ __launch_bounds__(WGM * WGN * 64, (BM == 256 && KT == 32) ? 4 : (BN == 160 ? 2 : 1)) void gemm_dma_kernel(GemmArgs p) {
  constexpr int EPI = EPI_PLAIN;
#include "gemm_dma_kernel.inc"
}
// The same kernel with the GEGLU fused into the store phase of its epilogue (EPI = EPI_GEGLU | EPI_GEGLU_BWD; gemm_common.h, write_tile): dense GEMM,
// plain staging.  The forward kind differs outside the epilogue in ONE place, the global B row of each DMA piece (geglu_col).
template <int BM, int BN, int WGM, int WGN, int NSTAGE, int KT, int EPI>
__global__ __launch_bounds__(WGM * WGN * 64, (BM == 256 && KT == 32) ? 4 : (BN == 160 ? 2 : 1)) void gemm_dma_geglu_kernel(GemmArgs p) {
  constexpr int MODE = 0;
  constexpr bool GENERAL = false;
#include "gemm_dma_kernel.inc"
}

// ------------------------------------------------------------------------------------------------
// 3x3 stride-1 convolution on 256-pixel ROW SEGMENTS, the A operand staged as STRIPS (round 6; the VAE's 128-channel level).
//
// gemm_dma_kernel<256, 128, ..., 32> fetches a 256-pixel x 32-channel A tile per (tap, channel chunk): the three taps of one kernel
// row read the SAME pixels shifted by one, three times through the CU's fill path (a timing probe that let two of three taps fetch
// nothing ran the 128 -> 128 conv at 512 x 512 in 1223 instead of 1430 us).  When a tile is 256 consecutive pixels of ONE image row
// (W % 256 == 0), the pixels x0 - 1 .. x0 + 256 of input row y + ky - 1 are staged ONCE per (ky, chunk) — a strip of 258 rows x 64
// bytes — and the taps kx = 0, 1, 2 read it at row offsets 0, 1, 2: the fragment read of output pixel r for tap kx is strip row
// r + kx (any 16 consecutive rows of the (r >> 2) & 3 slot swizzle are conflict-free, so the shift costs nothing in LDS).  A-side fill
// bytes and DMA instructions per MFMA drop 3 x / 2 x; the B side (weights, one 128 x 32 tile per tap and chunk) is unchanged.
//   LDS: two strip buffers of 24 pieces (384 rows; rows beyond 257 and pixels outside the image carry the out-of-range offset and
//   fetch nothing) + three B buffers = 72 KB, two workgroups per CU, the epilogue staging of gemm_dma_kernel on top of it.
//   Order of the K walk: ky, channel chunk, kx (B follows: column (3 ky + kx) Cin + 32 chunk): only the fp32 summation order differs.
//   Pipeline: sub-step j = (strip s, kx) issues B(j + 2) and, at kx = 0, strip s + 1; per wave 3 strip pieces + 1 B piece, so the
//   counted waits are vmcnt(1) / (4) / (1) for kx = 0 / 1 / 2 (what may still be in flight behind the B tile — and strip — the sub-step
//   needs), one barrier per sub-step as in the tile kernel.
// ------------------------------------------------------------------------------------------------
// WGN = 2: 256 x 128 tile, 8 waves, two workgroups per CU.  WGN = 4: 256 x 256 tile, 16 waves in ONE workgroup per CU — the same four waves
// per SIMD, a strip now feeds 256 output channels (half the A-side fill per flop again), and the waves split the issue work: waves 0-7
// stage the strips (3 pieces each per strip), waves 8-15 the 256 x 32 B tiles (2 pieces each per sub-step), each group with its own
// counted wait (vmcnt(0) once per strip / vmcnt(2) per sub-step).  Only WGN = 2 is instantiated: WGN = 4 measured equal to the ping-pong kernel it would
// replace (the LDS read port).  Its branches stay in the source: written out for 8 waves alone, conv_strip_kernel<2> compiles to a different instruction
// stream.  They go with the next change to this kernel that carries its own measurement.
template <int WGN>
__global__ __launch_bounds__(256 * WGN, 4) void conv_strip_kernel(GemmArgs p) {
  constexpr int BN = 64 * WGN, KT = 32, WM = 64, WN = 64, FM = 2, FN = 2;
  constexpr bool SPLIT = WGN == 4;                                   // issue roles split between wave groups
  constexpr int NBP = SPLIT ? 2 : 1;                                 // B pieces per issuing wave and sub-step
  constexpr int ASZ = 384 * KT, BSZ = BN * KT;                       // elements per strip / B buffer
  __shared__ __attribute__((aligned(16))) bf16_t smem[2 * ASZ + 3 * BSZ];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WGN, wn = wave % WGN;
  int tile_x, tile_y;
  xcd_tile(tile_x, tile_y, p.group_m);
  const int m0 = tile_y * 256, n0 = tile_x * BN;
  const int hw = p.Hin * p.Win;
  const int b = m0 / hw, rem = m0 - b * hw, y = rem / p.Win, x0 = rem - y * p.Win;
  // the tile's 256 output pixels and their strips of input row y + ky - 1 (+ ry): StripGeom (whole-row tiles: x0 = 0)
  const StripGeom sg(p.Win);
  const int ncc = p.Cin / KT, nstrip = 3 * ncc, nsub = 3 * nstrip;

  const __amdgpu_buffer_rsrc_t rs_a = cm_rsrc(p);                   // base lowered by one image row + one pixel (never touched: masked lanes)
  const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc((void*)p.B, 0, (int)p.b_bytes, 0x00020000);
  // strip pieces of this wave: piece q = wave + 8 i covers strip rows 16 q .. 16 q + 15; strip row j = input pixel x0 - 1 + j
  unsigned a_vo[3];
  int a_inv[3];                                  // bit ky set = this strip row reads padding (or nothing) for kernel row ky
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int j = 16 * (wave + 8 * i) + (lane >> 2);
    const int ry = j / sg.SW, xs = j - ry * sg.SW, ix = x0 - 1 + xs;      // written out: profiles/gemm_addressing_isa.txt
    const bool ok = ry < sg.nrows && ix >= 0 && ix < p.Win;
    a_vo[i] = (unsigned)(((ry * p.Win + xs) * p.Cin + ((lane & 3) ^ swz_slot<KT>(j)) * 8) * 2);
    int m = 0;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = y + ry + ky - 1;
      if (!(ok && iy >= 0 && iy < p.Hin)) m |= 1 << ky;
    }
    a_inv[i] = m;
  }
  const bool a_wave = !SPLIT || wave < 8, b_wave = !SPLIT || wave >= 8;      // (wave-uniform)
  const int bw = SPLIT ? wave - 8 : wave;                                     // B pieces of this wave: NBP bw .. NBP bw + NBP - 1
  unsigned b_vo[NBP];
#pragma unroll
  for (int i = 0; i < NBP; ++i) {
    const int r = 16 * (NBP * bw + i) + (lane >> 2);
    b_vo[i] = (b_wave && n0 + r < p.N) ? (unsigned)((((size_t)(n0 + r)) * p.ldb + ((lane & 3) ^ swz_slot<KT>(r)) * 8) * 2) : OOB;
  }
  // walkers (incremental: no division per issue)
  int a_ky = 0, a_cc = 0;                        // next strip to issue
  int b_ky = 0, b_cc = 0, b_kx = 0;              // next B tile to issue
  auto issue_a = [&](bf16_t* buf) __attribute__((always_inline)) {
    const int iy = y + a_ky - 1;
    // ((b H + iy) W + x0 - 1) Cin + 32 cc, against the lowered base: + (W + 1) Cin  ->  ((b H + iy + 1) W + x0) Cin + 32 cc  >= 0
    const int so = __builtin_amdgcn_readfirstlane((int)(((((long long)b * p.Hin + iy + 1) * p.Win + x0) * p.Cin + a_cc * KT) * 2));
#pragma unroll
    for (int i = 0; i < 3; ++i)      // the lane's offset, or all-ones (out of range) where the strip row is padding for this kernel row
      buf_dma16(rs_a, a_vo[i] | (unsigned)__builtin_amdgcn_sbfe(a_inv[i], (unsigned)a_ky, 1u), so, buf + (wave + 8 * i) * 512);
    if (++a_cc == ncc) { a_cc = 0; ++a_ky; }
  };
  auto issue_b = [&](bf16_t* buf) __attribute__((always_inline)) {
    const int so = __builtin_amdgcn_readfirstlane((((b_ky * 3 + b_kx) * p.Cin) + b_cc * KT) * 2);
#pragma unroll
    for (int i = 0; i < NBP; ++i) buf_dma16(rs_b, b_vo[i], so, buf + (NBP * bw + i) * 512);
    if (++b_kx == 3) { b_kx = 0; if (++b_cc == ncc) { b_cc = 0; ++b_ky; } }
  };

  f32x16 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int frow = lane & 31, fhi = lane >> 5;
  int a_off[3][FM][2], b_off[FN][2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        const int o = wm * WM + i * 32 + frow;                 // output pixel of the tile
        const int r = sg.frag_row(o, kx);         // its strip row for tap kx
        a_off[kx][i][ks] = frag_off<KT>(r, ks, fhi);
      }
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int r = wn * WN + j * 32 + frow;
      b_off[j][ks] = frag_off<KT>(r, ks, fhi);
    }
  }
  bf16_t* const Bs = smem + 2 * ASZ;
  if (a_wave) issue_a(smem);                     // strip 0
  if (b_wave) { issue_b(Bs); issue_b(Bs + BSZ); }      // B(0), B(1)

  auto sub = [&](auto par_, auto kx_, int s) __attribute__((always_inline)) {
    constexpr int PAR = decltype(par_)::value, KX = decltype(kx_)::value;
    const int j = 3 * s + KX;
    if (SPLIT) {
      if (a_wave) { if (KX == 0) wait_vmcnt<0>(); }             // strip s (issued three sub-steps ago) is this wave's only traffic
      else if (j + 1 == nsub) wait_vmcnt<0>();                  // the last B tile
      else wait_vmcnt<2>();                                     // B(j + 1) may still fly
    } else {
      if (s + 1 == nstrip && KX > 0) wait_vmcnt<0>();          // the last strip: nothing (or one B tile) behind the one needed
      else if (KX == 1) wait_vmcnt<4>();                        // strip s + 1 (3 pieces) and B(j + 1) may still fly
      else wait_vmcnt<1>();                                     // B(j + 1) may
    }
    loop_barrier();
    if (a_wave && KX == 0 && s + 1 < nstrip) issue_a(smem + (PAR ^ 1) * ASZ);
    if (b_wave && j + 2 < nsub) issue_b(Bs + ((KX + 2) % 3) * BSZ);
    const bf16_t* sa = smem + PAR * ASZ;
    const bf16_t* sb = Bs + KX * BSZ;
    bf16x8 af[2][FM], bfr[2][FN];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int i = 0; i < FM; ++i) af[ks][i] = *(const bf16x8*)(sa + a_off[KX][i][ks]);
#pragma unroll
      for (int jj = 0; jj < FN; ++jj) bfr[ks][jj] = *(const bf16x8*)(sb + b_off[jj][ks]);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int jj = 0; jj < FN; ++jj)
          acc[i][jj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ks][i], bfr[ks][jj], acc[i][jj], 0, 0, 0);
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  for (int s = 0; s < nstrip; s += 2) {
    sub(I0{}, I0{}, s); sub(I0{}, I1{}, s); sub(I0{}, I2{}, s);
    if (s + 1 < nstrip) { sub(I1{}, I0{}, s + 1); sub(I1{}, I1{}, s + 1); sub(I1{}, I2{}, s + 1); }
  }
  __syncthreads();   // all fragment reads done before the epilogue reuses the LDS
  if constexpr (SPLIT) {     // 16 staging areas of a whole wave tile would not fit the operand buffers: two row halves (as the tall gemm_dma tiles do)
    static_assert(4 * WGN * (WM / 2) * (WN + 8) <= 2 * ASZ + 3 * BSZ, "epilogue staging must fit");
    write_tile<WM / 2, WN, FM / 2, FN, false>(p, *(f32x16(*)[FM / 2][FN])(acc + 0), wave_stage<WM / 2, WN>(smem, wave), lane, m0 + wm * WM, n0 + wn * WN);
    __syncthreads();
    write_tile<WM / 2, WN, FM / 2, FN, false>(p, *(f32x16(*)[FM / 2][FN])(acc + FM / 2), wave_stage<WM / 2, WN>(smem, wave), lane, m0 + wm * WM + WM / 2, n0 + wn * WN);
  } else {
    write_tile<WM, WN, FM, FN, false>(p, acc, wave_stage<WM, WN>(smem, wave), lane, m0 + wm * WM, n0 + wn * WN);
  }
}
// may a 256 x 128 x 32 (WGN = 2) / 256 x 256 (WGN = 4, in place of the ping-pong kernel) conv launch go to conv_strip_kernel?
static bool strips_enabled() { static const bool on = getenv("E4T_CONV_NOSTRIP") == nullptr; return on; }          // A/B switch of both strip kernels
static bool strip_rows_ok(const GemmArgs& p) { return p.Win % 256 == 0 || (p.Win >= 16 && 256 % p.Win == 0 && p.Hin % (256 / p.Win) == 0); }      // row segments, or whole rows per tile (StripGeom)
static bool conv_strip_ok(const GemmArgs& p, int splitk, int batch) {
  return strips_enabled() && p.mode == E4T_CONV_S1 && p.chan_major && splitk == 1 && batch == 1 && strip_rows_ok(p) && p.Wout == p.Win && p.Hout == p.Hin &&
         p.Cin % 32 == 0 && p.K == 9 * p.Cin;
}

#ifdef DMA_TRACE
}  // namespace
extern "C" int e4t_debug_dma_trace(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dma_trace), sizeof(g_dma_trace));
}
namespace {
#endif

// ------------------------------------------------------------------------------------------------
// 256 x 256 x 64 "ping-pong" variant for the big, K-deep shapes (VAE / 1280-channel convs, FF GEMMs).
//
// The 128-wide tiles above need ~64 B/clk/CU of L2->LDS traffic at MFMA peak and hide latency by occupancy
// (2 workgroups x 8 waves); they top out near 1 PFLOP/s.  This one halves the operand traffic per flop and
// schedules explicitly instead:
//   * 8 waves = 2 groups (wr) x 4 column slices (wc), wave tile 128 x 64 (4 x 2 accumulators of 32x32);
//     wave w and w+4 share a SIMD, one from each group;
//   * a K-tile is consumed in 4 PHASES of 8 MFMAs: (rows 0-63 | 64-127 of the wave tile) x (k 0-31 | 32-63).
//     Each phase = [L: fragment ds_reads + one 16-KiB operand quarter DMA issue + counted vmcnt] barrier
//     [M: 8 MFMAs at raised priority] barrier.  Group 1 runs one barrier interval behind group 0, so on every
//     SIMD one wave is in its MFMA segment while the other does its LDS/DMA segment;
//   * the operand stream is cut in QUARTERS (A|B) x (k-lo|k-hi), 256 rows x 32 k = 16 KiB each, two buffers of four:
//     a quarter slot is re-staged exactly 2 phases after its last ds_read and first read >= 5 phases after its
//     issue, so the DMA has > 2500 clk of flight time and vmcnt never drains to 0 inside the loop
//     (each phase issues 2 DMA instructions per wave; vmcnt(8) after the issue = everything older than the 4
//     newest quarters has landed; a quarter is read one phase after the wait + barrier that retires it);
//   * quarter rows are 64 B: LDS slot p of row r holds logical 16-B chunk p ^ ((r >> 2) & 3) (source-side swizzle,
//     conflict-free ds_read_b128 for the 32x32x16 fragment lane groups).
// Requires K % 64 == 0 (no ragged K-tile); M / N edges are handled by zero rows and the bounds-checked epilogue.
// ------------------------------------------------------------------------------------------------
#ifdef PP_TRACE     // debug builds only (tools/pp_trace.sh): cycle stamps of one wave per group
__device__ unsigned long long g_pp_trace[2 * 6 * 64];
#ifdef PP_TRACE_MIN
#define PP_STAMP(slot) do { if ((slot) == 0 && tracing && tr_n < 64) tr[wr][tr_n * 6] = __builtin_readcyclecounter(); } while (0)
#else
#define PP_STAMP(slot) do { if (tracing && tr_n < 64) tr[wr][tr_n * 6 + (slot)] = __builtin_readcyclecounter(); } while (0)
#endif
#else
#define PP_STAMP(slot) do { } while (0)
#endif
// CM (round 5): the channel-chunk-major K order of the stride-1 3x3 convs is a compile-time property of the instantiation, and the K loop
// runs its steady state — every quarter issue unconditional — apart from the last tiles.  As a runtime flag (round 3) both walks lived in
// every phase: a branch on the flag per DMA issue, the tap-major offsets kept alive next to the channel-major ones (the wave-uniform
// A offset was parked in a VGPR and fetched back with v_readfirstlane per issue), and the "is there a tile left to stage" compare /
// select / branch chain in every phase: ~9 of the ~24 scalar instructions per 8-MFMA phase (ISA, profiles/r05_isa_pp_loop.txt).
template <int MODE, bool GENERAL = false, bool CM = false>
__global__ __launch_bounds__(512) void gemm_pp_kernel(GemmArgs p) {
  constexpr int BM = 256, BN = 256, HK = 32;
  constexpr int QUART = 256 * HK;                        // elements per quarter
  constexpr int EPI = 8 * 64 * (64 + 8);                 // write_tile staging: 8 waves x 64 x 72
  constexpr int SMEM = EPI > 8 * QUART ? EPI : 8 * QUART;
  __shared__ __attribute__((aligned(16))) bf16_t smem[SMEM];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
#ifdef PP_TRACE
  __shared__ unsigned long long tr[2][6 * 64];
  const bool tracing = blockIdx.x == 1 && blockIdx.y == 1 && blockIdx.z == 0 && wc == 0 && lane == 0;
  int tr_n = -32;       // skip the first 32 phases
#endif
  int tile_x, tile_y;
  xcd_tile(tile_x, tile_y, p.group_m);
  const int m0 = tile_y * BM, n0 = tile_x * BN;

  const KRange kr = batch_entry<BK>(p, p.K / BK);
  const int kt_begin = kr.begin, kt_end = kr.end;

  // Operands are addressed through buffer resources (buffer_load ... lds): a 32-bit per-lane byte offset that changes only
  // when the conv tap / concat source changes, plus a wave-uniform SGPR offset that walks K (+64 B per quarter).  Issuing a
  // quarter costs no VALU at all, and out-of-range rows / conv padding simply carry an out-of-range offset (the hardware
  // returns zeros) instead of a redirected pointer.
  constexpr bool cm = MODE != 0 && CM;               // channel-chunk-major K order (gemm_common.h, cm_step): launch_gemm picks the instantiation
  const __amdgpu_buffer_rsrc_t rs_a = cm ? cm_rsrc(p) : uniform_rsrc(p.A, p.a_bytes);
  const __amdgpu_buffer_rsrc_t rs_a2 = uniform_rsrc(p.A2 ? p.A2 : p.A, p.A2 ? p.a2_bytes : p.a_bytes);
  const __amdgpu_buffer_rsrc_t rs_b = uniform_rsrc(p.B, p.b_bytes);
  // DMA: one wave-instruction = 16 rows x 64 B; wave w feeds quarter rows 32w + 16j + (lane >> 2), j = 0, 1
  const int drow = lane >> 2, dslot = lane & 3;
  long long a_base[2];
  int a_oy[2], a_ox[2], a_kc[2];
  bool a_ok[2];
  unsigned b_vo[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int r = wave * 32 + j * 16 + drow;
    const int kc = (dslot ^ swz_slot<HK>(r)) * 8;
    const int gr = m0 + r;
    a_ok[j] = gr < p.M;
    a_kc[j] = kc;
    if (MODE == 0) {
      a_base[j] = (long long)gr; a_oy[j] = a_ox[j] = 0;
    } else {
      out_pixel(p, gr, a_base[j], a_oy[j], a_ox[j]);
    }
    const int gn = n0 + r;
    b_vo[j] = gn < p.N ? (unsigned)(((size_t)gn * p.ldb + kc) * 2) : OOB;
  }
  unsigned a_vo[2];
  if (cm) {                        // a_vo = the output position's own pixel (all taps), a_oy = inverted 9-bit tap validity mask
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      a_vo[j] = cm_center(p, a_base[j], a_oy[j], a_ox[j], a_kc[j]);
      a_oy[j] = cm_inv_mask(p, a_ok[j], a_oy[j], a_ox[j]);
    }
  }
  unsigned a_eff[2] = {0u, 0u};    // cm: the offsets of the K-tile whose quarters are being issued
  CmWalk wa, wb;                   // cm: one walker per operand stream (A and B are issued at different times)
  wa.init(kt_begin, BK); wb = wa;
  const int cm_table = cm ? cm_tap_table(p, lane) : 0;
  int a_so = 0, b_so = 0;          // wave-uniform byte offsets along K
  bool a_second = false;           // reading the second concat source
  auto place_a = [&](int k0) {
    if (MODE == 0) {
      int ld = p.lda, koff = k0;      // written out: profiles/gemm_addressing_isa.txt
      a_second = k0 >= p.K1;
      if (a_second) { ld = p.lda2; koff = k0 - p.K1; }
      a_so = __builtin_amdgcn_readfirstlane(koff * 2);          // (wave-uniform by construction; keeps the offset in an SGPR for the compiler)
#pragma unroll
      for (int j = 0; j < 2; ++j) a_vo[j] = a_ok[j] ? (unsigned)((a_base[j] * ld + a_kc[j]) * 2) : OOB;
    } else {
      const int tap = k0 / p.Cin;
      const int ci0 = k0 - tap * p.Cin;
      const int ky = tap / 3, kx = tap - ky * 3;
      a_so = __builtin_amdgcn_readfirstlane(ci0 * 2);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        int iy, ix;
        bool ok = a_ok[j];      // written out: profiles/gemm_addressing_isa.txt
        if (p.mode == E4T_CONV_S1) {
          iy = a_oy[j] + ky - 1; ix = a_ox[j] + kx - 1;
          ok = ok && iy >= 0 && iy < p.Hin && ix >= 0 && ix < p.Win;
        } else if (p.mode == E4T_CONV_S2) {
          iy = 2 * a_oy[j] + ky - 1; ix = 2 * a_ox[j] + kx - 1;
          ok = ok && iy >= 0 && iy < p.Hin && ix >= 0 && ix < p.Win;
        } else if (p.mode == E4T_CONV_UP2) {
          iy = a_oy[j] + ky - 1; ix = a_ox[j] + kx - 1;
          ok = ok && iy >= 0 && iy < 2 * p.Hin && ix >= 0 && ix < 2 * p.Win;
          iy >>= 1; ix >>= 1;
        } else if (p.mode == E4T_CONV_S2A) {
          iy = 2 * a_oy[j] + ky; ix = 2 * a_ox[j] + kx;
          ok = ok && iy < p.Hin && ix < p.Win;
        } else {
          const int sy = a_oy[j] + ky - 1, sx = a_ox[j] + kx - 1;
          ok = ok && sy >= 0 && sx >= 0 && !(sy & 1) && !(sx & 1);
          iy = sy >> 1; ix = sx >> 1;
          ok = ok && iy < p.Hin && ix < p.Win;
        }
        a_vo[j] = ok ? (unsigned)(((a_base[j] + (long long)iy * p.Win + ix) * p.Cin + a_kc[j]) * 2) : OOB;
      }
    }
  };
  // The A and B streams are each issued in increasing k (lo(t), hi(t), lo(t+1), ...): +64 bytes on the scalar offset per quarter.
  auto issue_a = [&](int kt, bool hi, bf16_t* dst) __attribute__((always_inline)) {
    if (cm) {                        // lo(t), hi(t), lo(t+1), ...: the walker advances after each hi
      if (!hi) {
        a_so = cm_a_so(cm_table, wa);
#pragma unroll
        for (int j = 0; j < 2; ++j) a_eff[j] = cm_row_off(a_vo[j], a_oy[j], wa);
      } else {
        a_so = __builtin_amdgcn_readfirstlane(a_so + HK * 2);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) buf_dma16(rs_a, a_eff[j], a_so, dst + (wave * 32 + j * 16) * HK);
      if (hi) wa.next(BK);
      return;
    }
    const int k0 = kt * BK;
    const bool fresh = !hi && (kt == kt_begin || (MODE == 0 ? k0 == p.K1 : (k0 % p.Cin) == 0));
    if (fresh) place_a(k0);
    else a_so = __builtin_amdgcn_readfirstlane(a_so + HK * 2);
#pragma unroll
    for (int j = 0; j < 2; ++j)
      buf_dma16(a_second ? rs_a2 : rs_a, a_vo[j], a_so, dst + (wave * 32 + j * 16) * HK);
  };
  auto issue_b = [&](int kt, bool hi, bf16_t* dst) __attribute__((always_inline)) {
    if (cm && !hi) b_so = cm_b_so(p, wb);
    else if (!cm && !hi && kt == kt_begin) b_so = kt * BK * 2;
    else b_so = __builtin_amdgcn_readfirstlane(b_so + HK * 2);
#pragma unroll
    for (int j = 0; j < 2; ++j)
      buf_dma16(rs_b, b_vo[j], b_so, dst + (wave * 32 + j * 16) * HK);
    if (cm && hi) wb.next(BK);
  };

  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int frow = lane & 31, fhi = lane >> 5;
  int a_off[4][2], b_off[2][2];     // fragment offsets inside a quarter (elements), [block][k-step of the half]
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = wr * 128 + i * 32 + frow;
      a_off[i][ks] = frag_off<HK>(r, ks, fhi);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = wc * 64 + j * 32 + frow;
      b_off[j][ks] = frag_off<HK>(r, ks, fhi);
    }
  }
  // quarter slots of buffer b: lo-A, lo-B, hi-A, hi-B at (4b + 0..3) * QUART
  issue_b(kt_begin, false, smem + 1 * QUART);
  issue_a(kt_begin, false, smem + 0 * QUART);
  issue_b(kt_begin, true, smem + 3 * QUART);
  issue_a(kt_begin, true, smem + 2 * QUART);
  if (kt_begin + 1 < kt_end) {
    issue_b(kt_begin + 1, false, smem + 5 * QUART);
    issue_a(kt_begin + 1, false, smem + 4 * QUART);
    wait_vmcnt<8>();               // 12 issued: the two lo quarters of the first K-tile have landed
  } else {
    wait_vmcnt<0>();
  }
  __builtin_amdgcn_s_barrier();

  bf16x8 af[2][2], bfr[2][2];
  auto phase = [&](auto Bc, auto Pc, auto ALLc, int kt) {
    constexpr int b = decltype(Bc)::value, ph = decltype(Pc)::value;
    constexpr bool ALL = decltype(ALLc)::value;      // steady state: every quarter this phase stages exists
    constexpr int kh = ph >> 1, mh = ph & 1;
    bf16_t* const buf = smem + b * 4 * QUART;
    bf16_t* const other = smem + (b ^ 1) * 4 * QUART;
    const bf16_t* const qa = buf + (kh * 2) * QUART;
    const bf16_t* const qb = qa + QUART;
    // ---- L segment ----
    PP_STAMP(0);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) af[i][ks] = *(const bf16x8*)(qa + a_off[mh * 2 + i][ks]);
    if (mh == 0) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) bfr[j][ks] = *(const bf16x8*)(qb + b_off[j][ks]);
    }
    bool staged;
    if (ph == 0)      { staged = ALL || kt + 1 < kt_end; if (staged) issue_b(kt + 1, true, other + 3 * QUART); }
    else if (ph == 1) { staged = ALL || kt + 1 < kt_end; if (staged) issue_a(kt + 1, true, other + 2 * QUART); }
    else if (ph == 2) { staged = ALL || kt + 2 < kt_end; if (staged) issue_b(kt + 2, false, buf + 1 * QUART); }
    else              { staged = ALL || kt + 2 < kt_end; if (staged) issue_a(kt + 2, false, buf + 0 * QUART); }
    PP_STAMP(1);
    if (ALL || staged) wait_vmcnt<8>(); else wait_vmcnt<0>();
    PP_STAMP(2);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    PP_STAMP(3);
    // ---- M segment ----
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[mh * 2 + i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][ks], bfr[j][ks], acc[mh * 2 + i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    PP_STAMP(4);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    PP_STAMP(5);
#ifdef PP_TRACE
    if (tracing || tr_n < 0) ++tr_n;
#endif
  };
  using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>;

  if (wr == 1) __builtin_amdgcn_s_barrier();        // group 1 runs one barrier interval behind group 0
  {
    using YES = std::true_type; using NO = std::false_type;
    int kt = kt_begin;
    for (; kt + 4 <= kt_end; kt += 2) {       // steady state: tiles kt + 2 and kt + 3 exist, nothing to decide
      phase(I0{}, I0{}, YES{}, kt); phase(I0{}, I1{}, YES{}, kt); phase(I0{}, I2{}, YES{}, kt); phase(I0{}, I3{}, YES{}, kt);
      phase(I1{}, I0{}, YES{}, kt + 1); phase(I1{}, I1{}, YES{}, kt + 1); phase(I1{}, I2{}, YES{}, kt + 1); phase(I1{}, I3{}, YES{}, kt + 1);
    }
    for (; kt + 2 <= kt_end; kt += 2) {
      phase(I0{}, I0{}, NO{}, kt); phase(I0{}, I1{}, NO{}, kt); phase(I0{}, I2{}, NO{}, kt); phase(I0{}, I3{}, NO{}, kt);
      phase(I1{}, I0{}, NO{}, kt + 1); phase(I1{}, I1{}, NO{}, kt + 1); phase(I1{}, I2{}, NO{}, kt + 1); phase(I1{}, I3{}, NO{}, kt + 1);
    }
    if (kt < kt_end) { phase(I0{}, I0{}, NO{}, kt); phase(I0{}, I1{}, NO{}, kt); phase(I0{}, I2{}, NO{}, kt); phase(I0{}, I3{}, NO{}, kt); }
  }
  if (wr == 0) __builtin_amdgcn_s_barrier();
  __syncthreads();   // every fragment read and every DMA is done before the epilogue reuses the LDS
#ifdef PP_TRACE
  if (tracing) for (int i = 0; i < 6 * 64; ++i) g_pp_trace[wr * 6 * 64 + i] = tr[wr][i];
#endif
  // two 64-row halves: keeps the (fully unrolled) epilogue at the size of the 128-wide kernels'
  write_tile<64, 64, 2, 2, GENERAL>(p, *(f32x16(*)[2][2])(acc + 0), wave_stage<64, 64>(smem, wave), lane, m0 + wr * 128, n0 + wc * 64);
  __syncthreads();
  write_tile<64, 64, 2, 2, GENERAL>(p, *(f32x16(*)[2][2])(acc + 2), wave_stage<64, 64>(smem, wave), lane, m0 + wr * 128 + 64, n0 + wc * 64);
  if constexpr (MODE == 0) {
    if (p.tail_rows) gemm_tail<8, GENERAL>(p, (float*)smem, wave, lane);
  }
}

// ------------------------------------------------------------------------------------------------
// gemm_pp_kernel for stride-1 3x3 convs with the A operand staged as STRIPS (round 6; see conv_strip_kernel for the idea and the probe
// behind it: a third of the A-side fill is worth 12-16 % to the ping-pong kernel on every conv shape of the step).
//
// Same machine — two groups of four waves alternating an LDS/DMA segment with an 8-MFMA segment, B quarters of 256 x 32 by LDS-DMA, the
// channel-chunk-major K order (K-tile kt = chunk kt / 9, tap kt % 9) — but the three K-tiles kx = 0, 1, 2 of one kernel row read ONE strip:
// the tile's 256 output pixels (a 256-pixel row segment, or 256 / W whole rows) of input row y + ky - 1, each image row widened by a pixel
// on both sides, as two HALF-STRIPS (k 0-31 | 32-63 of the 64-channel chunk; <= 288 rows x 64 B, staged as 24 pieces = 3 per wave, rows
// beyond the strip / outside the image fetch nothing).  The fragment of output pixel o for tap kx is strip row (o / w)(w + 2) + o % w + kx.
//   * LDS: [strip parity][k half] 4 x 24 KB + [B buffer][k half] 4 x 16 KB = 160 KB — all of it;
//   * issue stream per K-tile: ph0 B-hi(t + 1), ph2 B-lo(t + 2) as before; the A stream shrinks to ONE piece of each half of strip s + 1 in
//     phases g = 1, 3, 5 of the strip's twelve (g = 4 kx + ph): 18 instead of 24 DMA instructions per wave and three K-tiles, two per phase like
//     the B events beside them (issued as two bursts of three in g = 1 / 3 the kernel measured 1-2 % slower: the long L segment makes the other
//     wave group wait); a half-strip slot is re-staged >= 2 phases after its last read and first read >= 7 phases after its last piece's issue;
//   * the counted wait keeps the ping-pong kernel's rule — after a phase's issue, at most the pieces of the LAST FOUR issue events may be
//     outstanding — with events of 2 or 0 pieces: vmcnt(4, 6, 6, 8 | 8, 8, 8, 6 | 6, 4, 4, 4) over the 12 phases of a strip;
//   * 6 K-tiles per loop body (tap shift, strip parity and B buffer are compile-time in every phase); the last tiles run the same phases
//     with the "is there anything left to stage" decisions, draining the counter where an issue is skipped.
// Requires: E4T_CONV_S1, chan_major, Cin % 64 == 0, W % 256 == 0 or (256 % W == 0, W >= 16, H % (256 / W) == 0), a K range per split that
// starts and ends on a kernel row (ktiles_per_split % 3 == 0).  Results differ from gemm_pp_kernel's in nothing (same K order, same MFMAs).
// ------------------------------------------------------------------------------------------------
template <bool GENERAL>
__global__ __launch_bounds__(512) void gemm_pps_kernel(GemmArgs p) {
  constexpr int BM = 256, BN = 256, HK = 32;
  constexpr int QUART = 256 * HK;                        // elements per B quarter
  constexpr int HSTRIP = 384 * HK;                       // elements per half-strip (24 pieces)
  constexpr int A_EL = 4 * HSTRIP;
  constexpr int SMEM = A_EL + 4 * QUART;                 // 160 KB
  static_assert(8 * 64 * (64 + 8) <= SMEM, "write_tile staging must fit");
  __shared__ __attribute__((aligned(16))) bf16_t smem[SMEM];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  int tile_x, tile_y;
  xcd_tile(tile_x, tile_y, p.group_m);
  const int m0 = tile_y * BM, n0 = tile_x * BN;

  const int nkt = p.K / BK;
  const int bz = blockIdx.z / p.splitk, sz = blockIdx.z - bz * p.splitk;      // (not batch_entry(): batch == 1 here, only bias and C move)
  if (p.bias) p.bias += bz * p.strideBias;
  if (!p.reduce_batch) {
    if (p.flags & E4T_OUT_F32) p.C = (float*)p.C + bz * p.strideC;
    else p.C = (bf16_t*)p.C + bz * p.strideC;
  }
  const int kt_begin = sz * p.ktiles_per_split;
  int kt_end = kt_begin + p.ktiles_per_split;
  if (kt_end > nkt) kt_end = nkt;

  const int hw = p.Hin * p.Win;
  const int ib = m0 / hw, rem = m0 - ib * hw, y = rem / p.Win, x0 = rem - y * p.Win;
  const StripGeom sg(p.Win);
  const __amdgpu_buffer_rsrc_t rs_a = cm_rsrc(p);
  const __amdgpu_buffer_rsrc_t rs_b = uniform_rsrc(p.B, p.b_bytes);
  const int drow = lane >> 2, dslot = lane & 3;
  // half-strip pieces of this wave: piece q = wave + 8 i = strip rows 16 q .. 16 q + 15
  unsigned a_vo[3];
  int a_inv[3];                                  // bit ky set = this strip row is padding (or no row at all) for kernel row ky
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int j = 16 * (wave + 8 * i) + drow;
    const int ry = j / sg.SW, xs = j - ry * sg.SW, ix = x0 - 1 + xs;      // written out: profiles/gemm_addressing_isa.txt
    const bool ok = ry < sg.nrows && ix >= 0 && ix < p.Win && m0 < p.M;
    a_vo[i] = (unsigned)(((ry * p.Win + xs) * p.Cin + (dslot ^ ((j >> 2) & 3)) * 8) * 2);      // written out: profiles/gemm_addressing_isa.txt
    int m = 0;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = y + ry + ky - 1;
      if (!(ok && iy >= 0 && iy < p.Hin)) m |= 1 << ky;
    }
    a_inv[i] = m;
  }
  unsigned b_vo[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int r = wave * 32 + j * 16 + drow;
    const int gn = n0 + r;
    b_vo[j] = gn < p.N ? (unsigned)(((size_t)gn * p.ldb + (dslot ^ ((r >> 2) & 3)) * 8) * 2) : OOB;
  }
  CmWalk wb;                       // B stream: (tap, chunk) of the next K-tile to issue
  wb.init(kt_begin, BK);
  int b_so = 0;
  int a_ky = (kt_begin % 9) / 3, a_chb = (kt_begin / 9) * BK * 2;       // A stream: kernel row and chunk byte offset of the next strip to issue
  auto issue_b = [&](bool hi, bf16_t* dst) __attribute__((always_inline)) {
    if (!hi) b_so = cm_b_so(p, wb);
    else b_so = __builtin_amdgcn_readfirstlane(b_so + HK * 2);
#pragma unroll
    for (int j = 0; j < 2; ++j) buf_dma16(rs_b, b_vo[j], b_so, dst + (wave * 32 + j * 16) * HK);
    if (hi) wb.next(BK);
  };
  auto issue_strip = [&](bool hi, bf16_t* dst) __attribute__((always_inline)) {
    const int iy = y + a_ky - 1;
    // pixel (iy, x0 - 1) of image ib against the lowered base (+ (W + 1) Cin elements): ((ib H + iy + 1) W + x0) Cin  >= 0
    const int so = __builtin_amdgcn_readfirstlane((int)((((long long)ib * p.Hin + iy + 1) * p.Win + x0) * p.Cin * 2) + a_chb + (hi ? HK * 2 : 0));
#pragma unroll
    for (int i = 0; i < 3; ++i)
      buf_dma16(rs_a, a_vo[i] | (unsigned)__builtin_amdgcn_sbfe(a_inv[i], (unsigned)a_ky, 1u), so, dst + (wave + 8 * i) * 512);
    if (hi && ++a_ky == 3) { a_ky = 0; a_chb += BK * 2; }
  };
  // piece i of BOTH halves of the next strip per call (three calls per strip, in phase 1 of the kx = 0, 1, 2 tiles... see phase())
  auto issue_strip_piece = [&](auto Ic, bool last, bf16_t* dst_lo) __attribute__((always_inline)) {
    constexpr int i = decltype(Ic)::value;
    const int iy = y + a_ky - 1;
    const int so = __builtin_amdgcn_readfirstlane((int)((((long long)ib * p.Hin + iy + 1) * p.Win + x0) * p.Cin * 2) + a_chb);
    const unsigned vo = a_vo[i] | (unsigned)__builtin_amdgcn_sbfe(a_inv[i], (unsigned)a_ky, 1u);
    buf_dma16(rs_a, vo, so, dst_lo + (wave + 8 * i) * 512);
    buf_dma16(rs_a, vo, so + HK * 2, dst_lo + HSTRIP + (wave + 8 * i) * 512);
    if (last && ++a_ky == 3) { a_ky = 0; a_chb += BK * 2; }
  };

  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int frow = lane & 31, fhi = lane >> 5;
  int a_off[3][4][2], b_off[2][2];     // fragment offsets inside a half-strip (per tap shift) / a quarter (elements)
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int o = wr * 128 + i * 32 + frow;
        const int r = sg.frag_row(o, kx);
        a_off[kx][i][ks] = frag_off<HK>(r, ks, fhi);
      }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = wc * 64 + j * 32 + frow;
      b_off[j][ks] = frag_off<HK>(r, ks, fhi);
    }
  }
  bf16_t* const Bq = smem + A_EL;      // B quarter (buffer bb, half kh) at Bq + (2 bb + kh) QUART; half-strip (parity sp, half kh) at smem + (2 sp + kh) HSTRIP
  issue_strip(false, smem);
  issue_strip(true, smem + HSTRIP);
  issue_b(false, Bq);
  issue_b(true, Bq + QUART);
  if (kt_begin + 1 < kt_end) issue_b(false, Bq + 2 * QUART);
  wait_vmcnt<0>();                 // (once per workgroup: the counted waits of the loop start from an empty queue)
  __builtin_amdgcn_s_barrier();

  bf16x8 af[2][2], bfr[2][2];
  using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>;
  auto phase = [&](auto Bc, auto Pc, auto ALLc, auto KXc, auto SPc, int kt) {
    constexpr int bb = decltype(Bc)::value, ph = decltype(Pc)::value, KX = decltype(KXc)::value, SP = decltype(SPc)::value;
    constexpr bool ALL = decltype(ALLc)::value;      // steady state: everything this phase stages exists
    constexpr int kh = ph >> 1, mh = ph & 1;
    const bf16_t* const qa = smem + (2 * SP + kh) * HSTRIP;
    const bf16_t* const qb = Bq + (2 * bb + kh) * QUART;
    // ---- L segment ----
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) af[i][ks] = *(const bf16x8*)(qa + a_off[KX][mh * 2 + i][ks]);
    if (mh == 0) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) bfr[j][ks] = *(const bf16x8*)(qb + b_off[j][ks]);
    }
    bool staged = true;              // phases that issue nothing by design keep the pattern's count
    if (ph == 0)      { staged = ALL || kt + 1 < kt_end; if (staged) issue_b(true, Bq + (2 * (bb ^ 1) + 1) * QUART); }
    else if (ph == 2) { staged = ALL || kt + 2 < kt_end; if (staged) issue_b(false, Bq + (2 * bb + 0) * QUART); }
    // one piece of each half of the next strip in phases g = 1, 3, 5 of the strip's twelve (both halves land >= 5 events before their first read at g = 12 / 14)
    else if (4 * KX + ph == 1) { staged = ALL || kt + 3 < kt_end; if (staged) issue_strip_piece(I0{}, false, smem + 2 * (SP ^ 1) * HSTRIP); }
    else if (4 * KX + ph == 3) { staged = ALL || kt + 3 < kt_end; if (staged) issue_strip_piece(I1{}, false, smem + 2 * (SP ^ 1) * HSTRIP); }
    else if (4 * KX + ph == 5) { staged = ALL || kt + 2 < kt_end; if (staged) issue_strip_piece(I2{}, true, smem + 2 * (SP ^ 1) * HSTRIP); }
    constexpr int G_ = 4 * KX + ph;
    constexpr int NW_ = G_ == 0 ? 4 : G_ <= 2 ? 6 : G_ <= 6 ? 8 : G_ <= 8 ? 6 : 4;
    if (ALL || staged) wait_vmcnt<NW_>(); else wait_vmcnt<0>();
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    // ---- M segment ----
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[mh * 2 + i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][ks], bfr[j][ks], acc[mh * 2 + i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };
  // K-tile i of a 6-tile body: B buffer i & 1, tap shift i % 3, strip parity (i / 3) & 1
  auto ktile = [&](auto Bc, auto KXc, auto SPc, auto ALLc, int kt) __attribute__((always_inline)) {
    phase(Bc, I0{}, ALLc, KXc, SPc, kt); phase(Bc, I1{}, ALLc, KXc, SPc, kt); phase(Bc, I2{}, ALLc, KXc, SPc, kt); phase(Bc, I3{}, ALLc, KXc, SPc, kt);
  };

  if (wr == 1) __builtin_amdgcn_s_barrier();        // group 1 runs one barrier interval behind group 0
  {
    using YES = std::true_type; using NO = std::false_type;
    int kt = kt_begin;
    for (; kt + 8 <= kt_end; kt += 6) {       // steady state: everything the six tiles stage (up to B-lo of tile kt + 7, the strip of kt + 6) exists
      ktile(I0{}, I0{}, I0{}, YES{}, kt);     ktile(I1{}, I1{}, I0{}, YES{}, kt + 1); ktile(I0{}, I2{}, I0{}, YES{}, kt + 2);
      ktile(I1{}, I0{}, I1{}, YES{}, kt + 3); ktile(I0{}, I1{}, I1{}, YES{}, kt + 4); ktile(I1{}, I2{}, I1{}, YES{}, kt + 5);
    }
    if (kt < kt_end) { ktile(I0{}, I0{}, I0{}, NO{}, kt); ktile(I1{}, I1{}, I0{}, NO{}, kt + 1); ktile(I0{}, I2{}, I0{}, NO{}, kt + 2); kt += 3; }
    if (kt < kt_end) { ktile(I1{}, I0{}, I1{}, NO{}, kt); ktile(I0{}, I1{}, I1{}, NO{}, kt + 1); ktile(I1{}, I2{}, I1{}, NO{}, kt + 2); kt += 3; }
  }
  if (wr == 0) __builtin_amdgcn_s_barrier();
  __syncthreads();   // every fragment read and every DMA is done before the epilogue reuses the LDS
  write_tile<64, 64, 2, 2, GENERAL>(p, *(f32x16(*)[2][2])(acc + 0), wave_stage<64, 64>(smem, wave), lane, m0 + wr * 128, n0 + wc * 64);
  __syncthreads();
  write_tile<64, 64, 2, 2, GENERAL>(p, *(f32x16(*)[2][2])(acc + 2), wave_stage<64, 64>(smem, wave), lane, m0 + wr * 128 + 64, n0 + wc * 64);
}
// may a 256 x 256 ping-pong conv launch go to gemm_pps_kernel?
static bool conv_pps_ok(const GemmArgs& p, int /*splitk*/, int batch) {
  return strips_enabled() && p.mode == E4T_CONV_S1 && p.chan_major && batch == 1 && strip_rows_ok(p) && p.Wout == p.Win && p.Hout == p.Hin && p.Cin % 64 == 0 &&
         p.K == 9 * p.Cin && p.ktiles_per_split % 3 == 0 && p.M % 256 == 0;
}

// ------------------------------------------------------------------------------------------------
// 256 x 320 ping-pong, phases = (k half) x (16-wide k step)      [round 3; the template also builds BN = 256, measured = gemm_pp_kernel]
//
// The same machine as gemm_pp_kernel — two groups of four waves alternating an LDS/DMA segment with an MFMA segment, operand
// quarters of 32 k moved by LDS-DMA, counted vmcnt — with the K-tile cut along K instead of along the wave tile's rows: a phase is
// one 16-wide k step over the WHOLE wave tile.  Every phase then reads the same number of fragments (FM + FN ds_read_b128 for
// FM x FN MFMAs) instead of alternating 8 / 4, holds one k step of fragments in registers instead of two (24 instead of 32 VGPRs
// at BN = 256), and — what it was written for — makes a 256 x 320 tile fit: 8 waves = 4 (rows) x 2 (columns), wave tile 64 x 160
// (2 x 5 accumulators = 160 VGPRs + 28 fragment registers), 10 MFMAs per phase.  A 320-wide tile covers the UNet's 320 / 640 /
// 960 / 1280 / 1920 / 2560-channel layers without N padding at 0.93 KB of LDS traffic per MFMA (fragment reads + DMA writes), where
// the 128 x 160 tile moves 1.69 KB (the GEMM family is bound by LDS traffic, not by the DMA path or the MFMA rate).
//   * quarters: A = 256 rows x 32 k (2 DMA instructions per wave), B = BN rows x 32 k (BN = 320: 20 pieces, 3 per wave in waves
//     0-3, 2 in waves 4-7); two buffers x [A-lo | B-lo | A-hi | B-hi] = 128 / 144 KiB;
//   * phases 0, 1 read the lo quarters, 2, 3 the hi quarters.  A slot is re-staged no earlier than two phases after its last read
//     (the trailing group's reads), so the issue stream runs  ph1: B-hi(t+1)  ph2: A-hi(t+1)  ph3: B-lo(t+2)  ph0': A-lo(t+2)
//     (A-lo of tile t+2 is issued in the first phase of tile t+1); every quarter is first read >= 3 phases after its issue, and
//     "at most the 3 newest quarters outstanding" after each issue is exactly what the next phase needs landed — 2 A + 1 B quarters
//     after an even phase, 1 A + 2 B after an odd one (instruction counts differ per wave at BN = 320).
// Requires K % 64 == 0.  Same epilogue code as every other kernel: results are bit-identical to theirs.
// ------------------------------------------------------------------------------------------------
template <int MODE, int BN, bool GENERAL>
__global__ __launch_bounds__(512) void gemm_pq_kernel(GemmArgs p) {
  constexpr int EPI = EPI_PLAIN;
#include "gemm_pq_kernel.inc"
}
// (the fused GEGLU epilogues, as gemm_dma_geglu_kernel)
template <int BN, int EPI>
__global__ __launch_bounds__(512) void gemm_pq_geglu_kernel(GemmArgs p) {
  constexpr int MODE = 0;
  constexpr bool GENERAL = false;
#include "gemm_pq_kernel.inc"
}

#ifdef PP_TRACE
}  // namespace
extern "C" int e4t_debug_pp_trace(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pp_trace), sizeof(g_pp_trace));
}
namespace {
#endif

// ------------------------------------------------------------------------------------------------
// TN variant: C[M, N] = alpha * A^T . B with A = [K][M], B = [K][N] row-major bf16 — the contraction runs over the ROWS.
// This is the weight gradient dW = dY^T . X of every linear layer as the tensors lie in memory; the NT kernels above need
// both operands transposed first (two extra passes over dY and X per weight gradient).
//   * operand tiles are [64 k-rows][128 columns] (256-B rows), still moved by LDS-DMA, 4 rows per wave-instruction;
//   * the MFMA fragments (lane = output row / column, 8 consecutive k) are gathered with gfx950's transposing LDS read
//     ds_read_b64_tr_b16: within a 16-lane group, source lane i' supplies 4 contiguous elements and output lane i receives,
//     in slot j, element (i % 4) of source lane 4j + i / 4 (probed on hardware: tools/probe/tr_probe.hip).  Pointing
//     source lane i' at T[kbase + i'/4][n0 + 4 (i' % 4)] therefore hands lane i the column n0 + i of rows kbase .. kbase+3;
//     two such reads (rows +0 and +4) make one bf16x8 operand;
//   * bank conflicts: a 32-lane half reads 64 contiguous bytes from each of 4 consecutive rows; rows are 256 B apart = the
//     same banks, so 32-byte unit u of row r is stored at unit u ^ (2 (r & 3)) (swizzle applied on the DMA source side).
// 128 x 128 x 64 tile, 8 waves (wave tile 32 x 64), two LDS buffers, one barrier per K-tile, as the NT kernel.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void gemm_tn_kernel(GemmArgs p) {
  constexpr int BM = 128, BN = 128, WGN = 2, WM = 32, WN = 64, FN = 2;
  constexpr int OPER = BK * 128;                 // elements per operand tile: 64 rows x 128 columns
  constexpr int TILE = 2 * OPER;
  __shared__ __attribute__((aligned(16))) bf16_t smem[2 * TILE];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WGN, wn = wave % WGN;
  int tile_x, tile_y, sz = blockIdx.z;           // sz: split index (no batching in this variant)
  if (p.xcd3) { xcd_tile3(tile_x, tile_y, sz); p.zslab = sz; }
  else xcd_tile(tile_x, tile_y, p.group_m);
  const int m0 = tile_y * BM, n0 = tile_x * BN;

  const int nkt = (p.K + BK - 1) / BK;
  const int kt_begin = sz * p.ktiles_per_split;
  int kt_end = kt_begin + p.ktiles_per_split;
  if (kt_end > nkt) kt_end = nkt;

  // buffer-resource addressing as in the NT kernels: per-lane byte offset (row in piece, swizzled column chunk) fixed for the
  // whole loop, the wave-uniform scalar offset walks the contraction rows (+64 rows per K-tile); rows beyond K and columns
  // beyond M / N carry an out-of-range offset and read as zero
  const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, (int)p.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc((void*)p.B, 0, (int)p.b_bytes, 0x00020000);
  // DMA: piece q = 4 tile rows; wave w feeds pieces 2w, 2w+1 of each operand.  lane -> (row in piece, physical 16-B chunk)
  const int prow = lane >> 4, pchunk = lane & 15;
  const int lchunk = (((pchunk >> 1) ^ (2 * prow)) << 1) | (pchunk & 1);      // logical chunk stored at this physical slot
  const bool a_col_ok = m0 + lchunk * 8 < p.M, b_col_ok = n0 + lchunk * 8 < p.N;
  unsigned a_col[2], b_col[2], a_vo[2], b_vo[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = (wave * 2 + i) * 4 + prow;              // tile row of this lane in piece i
    a_col[i] = a_col_ok ? (unsigned)(((size_t)r * p.lda + m0 + lchunk * 8) * 2) : OOB;
    b_col[i] = b_col_ok ? (unsigned)(((size_t)r * p.ldb + n0 + lchunk * 8) * 2) : OOB;
  }
  int a_so = 0, b_so = 0;
  auto issue_tile = [&](int kt, bf16_t* buf) __attribute__((always_inline)) {
    if (kt == kt_begin || (kt + 1) * BK > p.K) {          // first tile, or the ragged last one: mask the rows beyond K
      a_so = kt * BK * p.lda * 2; b_so = kt * BK * p.ldb * 2;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const bool row_ok = kt * BK + (wave * 2 + i) * 4 + prow < p.K;
        a_vo[i] = row_ok ? a_col[i] : OOB;
        b_vo[i] = row_ok ? b_col[i] : OOB;
      }
    } else {
      a_so += BK * p.lda * 2; b_so += BK * p.ldb * 2;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) buf_dma16(rs_a, a_vo[i], a_so, buf + (wave * 2 + i) * 512);
#pragma unroll
    for (int i = 0; i < 2; ++i) buf_dma16(rs_b, b_vo[i], b_so, buf + OPER + (wave * 2 + i) * 512);
  };

  f32x16 acc[1][FN];
#pragma unroll
  for (int j = 0; j < FN; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][j][r] = 0.f;

  // fragment gather addresses (elements) inside an operand tile for k-step 0, rows +0; +4 rows = +512, next k-step = +2048
  const int g16 = lane >> 4, il = lane & 15;
  const int frow = (g16 >> 1) * 8 + (il >> 2);
  auto frag_off = [&](int col0) {                 // col0: first of the 32 tile columns of the MFMA block
    const int col = col0 + 16 * (g16 & 1) + 4 * (il & 3);
    const int unit = (col >> 4) ^ (2 * (il >> 2));
    return frow * 128 + unit * 16 + (col & 15);
  };
  const int a_off = frag_off(wm * WM);
  int b_off[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) b_off[j] = OPER + frag_off(wn * WN + j * 32);

  if (kt_begin < kt_end) issue_tile(kt_begin, smem);
  auto body = [&](auto CURc, int kt) {
    constexpr int CUR = decltype(CURc)::value;
    wait_vmcnt<0>();
    loop_barrier();
    const bf16_t* st = smem + CUR * TILE;
    bf16x8 af[2], bfr[2][FN];
    af[0] = tr_frag(st + a_off, st + a_off + 512);
#pragma unroll
    for (int j = 0; j < FN; ++j) bfr[0][j] = tr_frag(st + b_off[j], st + b_off[j] + 512);
    if (kt + 1 < kt_end) issue_tile(kt + 1, smem + (CUR ^ 1) * TILE);
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      const int c = ks & 1, n = c ^ 1;
      if (ks + 1 < BK / 16) {
        af[n] = tr_frag(st + a_off + (ks + 1) * 2048, st + a_off + (ks + 1) * 2048 + 512);
#pragma unroll
        for (int j = 0; j < FN; ++j) bfr[n][j] = tr_frag(st + b_off[j] + (ks + 1) * 2048, st + b_off[j] + (ks + 1) * 2048 + 512);
      }
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[c], bfr[c][j], acc[0][j], 0, 0, 0);
    }
  };
  {
    int kt = kt_begin;
    for (; kt + 2 <= kt_end; kt += 2) {
      body(std::integral_constant<int, 0>{}, kt);
      body(std::integral_constant<int, 1>{}, kt + 1);
    }
    if (kt < kt_end) body(std::integral_constant<int, 0>{}, kt);
  }
  __syncthreads();
  write_tile<WM, WN, 1, FN>(p, acc, wave_stage<WM, WN>(smem, wave), lane, m0 + wm * WM, n0 + wn * WN);
}

// sums `nz` consecutive partial slabs starting at slab blockIdx.y*nz, then runs the epilogue for batch entry blockIdx.y
__global__ __launch_bounds__(256) void splitk_reduce_kernel(GemmArgs p, int nz) {
  const size_t total = (size_t)p.M * p.N;
  const int bz = blockIdx.y;
  if (!p.reduce_batch) {
    if (p.bias) p.bias += bz * p.strideBias;
    if (p.flags & E4T_OUT_F32) p.C = (float*)p.C + bz * p.strideC;
    else p.C = (bf16_t*)p.C + bz * p.strideC;
  }
  const float* ws = p.ws + (size_t)bz * nz * total;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    float v = 0.f;
    for (int z = 0; z < nz; ++z) v += ws[(size_t)z * total + idx];
    const int row = (int)(idx / p.N), col = (int)(idx - (size_t)row * p.N);
    epilogue_store(p, v, row, col);
  }
}

// The same reduction for the common case — bf16 C, N and every leading dimension a multiple of 8, no accumulate — with 8
// columns per thread: the partial slabs are read as 2 x float4 per split with ALL splits of a trip in flight (the scalar
// version above walks them one 4-byte load at a time and answers the guarded bias / row-bias / residual loads of
// epilogue_store with one memory round trip each), bias / row bias / residual as 32- / 16-byte vectors, C as one 16-byte store.
// Same arithmetic, same summation order (z ascending), single rounding.
__global__ __launch_bounds__(256) void splitk_reduce8_kernel(GemmArgs p, int nz) {
  const int n8 = p.N >> 3;
  const size_t total = (size_t)p.M * p.N, total8 = (size_t)p.M * n8;
  const int bz = blockIdx.y;
  if (!p.reduce_batch) {
    if (p.bias) p.bias += bz * p.strideBias;
    p.C = (bf16_t*)p.C + bz * p.strideC;
  }
  const float* ws = p.ws + (size_t)bz * nz * total;
  const bf16_t* Rb = (const bf16_t*)p.residual;
  for (size_t i8 = (size_t)blockIdx.x * 256 + threadIdx.x; i8 < total8; i8 += (size_t)gridDim.x * 256) {
    const int row = (int)(i8 / n8), c8 = (int)(i8 - (size_t)row * n8) * 8;
    const size_t idx = (size_t)row * p.N + c8;
    float bi[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, rb[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, rs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (p.bias) { const float4 a = *(const float4*)(p.bias + c8), b = *(const float4*)(p.bias + c8 + 4); bi[0] = a.x; bi[1] = a.y; bi[2] = a.z; bi[3] = a.w; bi[4] = b.x; bi[5] = b.y; bi[6] = b.z; bi[7] = b.w; }
    if (p.rowbias) {
      const float* q = p.rowbias + (size_t)(row / p.rows_per_batch) * p.ldrb + c8;
      const float4 a = *(const float4*)q, b = *(const float4*)(q + 4);
      rb[0] = a.x; rb[1] = a.y; rb[2] = a.z; rb[3] = a.w; rb[4] = b.x; rb[5] = b.y; rb[6] = b.z; rb[7] = b.w;
    }
    if (Rb) unpack8(*(const uint4*)(Rb + (size_t)row * p.ldr + c8), rs);
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int z0 = 0; z0 < nz; z0 += 4) {
      float4 lo[4], hi[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float* q = ws + (size_t)min(z0 + u, nz - 1) * total + idx;
        lo[u] = *(const float4*)q; hi[u] = *(const float4*)(q + 4);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float w = z0 + u < nz ? 1.f : 0.f;
        v[0] += lo[u].x * w; v[1] += lo[u].y * w; v[2] += lo[u].z * w; v[3] += lo[u].w * w;
        v[4] += hi[u].x * w; v[5] += hi[u].y * w; v[6] += hi[u].z * w; v[7] += hi[u].w * w;
      }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float x = v[k] * p.alpha + bi[k] + rb[k];
      if (p.flags & E4T_ACT_GELU) x = gelu_f(x);
      v[k] = x + rs[k];
    }
    *(uint4*)((bf16_t*)p.C + (size_t)row * p.ldc + c8) = pack8(v);
  }
}

// ... and for fp32 C without bias / row bias / residual / activation — every weight-gradient GEMM (gemm_tn_kernel, the batched head
// gradients): 4 columns per thread, float4 loads of all splits of a trip in flight, optional accumulate into C.  The scalar kernel
// above ran these at 1.2-3.4 TB/s (one 4-byte load per split and element: profiles/r04_prefetch_off_roofline_per_shape.csv, e.g.
// M320 N320 nz32 11.1 us, M16 N1280 nz129 35.8 us).  Same summation order (z ascending).
__global__ __launch_bounds__(256) void splitk_reduce4f_kernel(GemmArgs p, int nz) {
  const int n4 = p.N >> 2;
  const size_t total = (size_t)p.M * p.N, total4 = (size_t)p.M * n4;
  const int bz = blockIdx.y;
  float* Cf = (float*)p.C + (p.reduce_batch ? 0 : bz * p.strideC);
  const float* ws = p.ws + (size_t)bz * nz * total;
  for (size_t i4 = (size_t)blockIdx.x * 256 + threadIdx.x; i4 < total4; i4 += (size_t)gridDim.x * 256) {
    const int row = (int)(i4 / n4), c4 = (int)(i4 - (size_t)row * n4) * 4;
    const size_t idx = (size_t)row * p.N + c4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int z0 = 0; z0 < nz; z0 += 8) {
      float4 t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = *(const float4*)(ws + (size_t)min(z0 + u, nz - 1) * total + idx);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float w = z0 + u < nz ? 1.f : 0.f;
        v.x += t[u].x * w; v.y += t[u].y * w; v.z += t[u].z * w; v.w += t[u].w * w;
      }
    }
    float4* c = (float4*)(Cf + (size_t)row * p.ldc + c4);
    float4 o = make_float4(v.x * p.alpha, v.y * p.alpha, v.z * p.alpha, v.w * p.alpha);
    if (p.flags & E4T_ACCUM) { const float4 a = *c; o.x += a.x; o.y += a.y; o.z += a.z; o.w += a.w; }
    *c = o;
  }
}

// ---- host half: ONE variant table drives tile choice (plan_gemm), launch and launch log (launch_gemm) -------------------------------------
int device_cu_count() {
  static const int ncu = [] {
    int dev = 0, n = 0;
    return hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0 ? n : 256;
  }();
  return ncu;
}

bool dma_allowed() { static const bool on = getenv("E4T_GEMM_REGSTAGE") == nullptr; return on; }      // A/B switch: register-staged reference kernel
// A kernel entry point and the symbol text rocprofv3 prints for it, from ONE macro invocation so that the launch log cannot name another
// kernel than the one launched: KERNEL(512, gemm_pp_kernel, 1, false, true) is {&gemm_pp_kernel<1, false, true>, "gemm_pp_kernel<1, false, true>", 512 threads}.
struct KernelEntry { void (*fn)(GemmArgs); const char* text; int threads; };      // text == nullptr: not instantiated
#define KERNEL(threads, name, ...) {&name<__VA_ARGS__>, #name "<" #__VA_ARGS__ ">", threads}
#define NO_KERNEL {nullptr, nullptr, 0}
enum : unsigned {
  CAP_STAGED = 1u << 0,      // the LDS depth is a template argument: hints 3xxx / 4xxx and the cost model choose among this tile's rows
  CAP_BUF = 1u << 1,         // LDS-DMA through buffer resources (32-bit byte offsets): operands below 4 GB, not under E4T_GEMM_REGSTAGE
  CAP_COLSTATS = 1u << 2,    // its bf16 single-pass epilogue produces column statistics
  CAP_SPLITK = 1u << 3,      // accepts split-K (grid.z)
  CAP_WHOLE_K = 1u << 4,     // needs whole 64-wide K-tiles (of each source of a two-source A)
  CAP_WHOLE_N = 1u << 5,     // needs N % tn == 0 (ragged N is only exercised for the narrower tiles)
  CAP_TAIL = 1u << 6,        // carries gemm_tail() (plan_gemm_tail)
  CAP_PANELS = 1u << 7,      // carries row panels
  CAP_ONE_PER_CU = 1u << 8,  // one 512-thread workgroup per CU: the "ping-pong" split-K rule
  CAP_GEGLU = 1u << 9,       // carries the fused GEGLU epilogues (Variant::geglu; E4T_EPI_GEGLU / E4T_EPI_GEGLU_BWD)
  CAP_DMA = CAP_BUF | CAP_COLSTATS | CAP_SPLITK,
};
// A conv launch of the row goes to a strip-staged kernel instead when ok(p, splitk, batch) holds at launch time.
struct StripAlt { bool (*ok)(const GemmArgs&, int, int); KernelEntry k[2]; };      // k[GENERAL]
struct Variant {
  int tile, kt, stages, tm, tn;      // the public tile code is `tile`, 1000 * stages + tile for 3 / 4 stages of a CAP_STAGED tile, 5000 + tile for kt == 32
  unsigned caps;
  KernelEntry gemm[2], conv[2], conv_cm[2];      // [GENERAL]; conv_cm: channel-major K order as a template argument (else a run-time flag)
  StripAlt alt;
  KernelEntry geglu[2];      // [EPI_GEGLU - 1], [EPI_GEGLU_BWD - 1]: dense GEMM with the GEGLU in the store phase (CAP_GEGLU)
};

// ---- the variant table.  How to add a variant: (1) write its kernel above, signature void(GemmArgs); (2) add ONE row here — tile code, tile shape, what it can
// do, its instantiations; (3) add the rule that chooses it to choose_tile() with the measurement that justifies it.  Everything else
// (hints, capability fallback, split-K, launch, launch log, e4t_gemm_plan) follows from the row.
#define DMA_FN(nt, bm, bn, wgm, wgn, st, kt) {KERNEL(nt, gemm_dma_kernel, bm, bn, wgm, wgn, 0, st, false, kt), NO_KERNEL}, \
                                             {KERNEL(nt, gemm_dma_kernel, bm, bn, wgm, wgn, 1, st, false, kt), NO_KERNEL}
#define DMA_FN_GENERAL(nt, bm, bn, wgm, wgn, st)                                                                                  \
  {KERNEL(nt, gemm_dma_kernel, bm, bn, wgm, wgn, 0, st, false, 64), KERNEL(nt, gemm_dma_kernel, bm, bn, wgm, wgn, 0, st, true, 64)}, \
  {KERNEL(nt, gemm_dma_kernel, bm, bn, wgm, wgn, 1, st, false, 64), KERNEL(nt, gemm_dma_kernel, bm, bn, wgm, wgn, 1, st, true, 64)}
// (the epilogue kind is spelled as its number, 1 = EPI_GEGLU, 2 = EPI_GEGLU_BWD: the text is the kernel symbol as a trace shows it)
#define DMA_GEGLU(nt, bm, bn, wgm, wgn, st, kt) {KERNEL(nt, gemm_dma_geglu_kernel, bm, bn, wgm, wgn, st, kt, 1), KERNEL(nt, gemm_dma_geglu_kernel, bm, bn, wgm, wgn, st, kt, 2)}
#define DMA_GEGLU_F(nt, bm, bn, wgm, wgn, st, kt) {KERNEL(nt, gemm_dma_geglu_kernel, bm, bn, wgm, wgn, st, kt, 1), NO_KERNEL}
#define DMA_GEGLU_B(nt, bm, bn, wgm, wgn, st, kt) {NO_KERNEL, KERNEL(nt, gemm_dma_geglu_kernel, bm, bn, wgm, wgn, st, kt, 2)}
#define REG_FN(bm, bn, mode) {{&gemm_kernel<bm, bn, 2, 2, mode>, "gemm_kernel", 256}, {&gemm_kernel<bm, bn, 2, 2, mode>, "gemm_kernel", 256}}
static const Variant kVariants[] = {
    // 64 / 128 / 160 tiles: 2 LDS stages and 2 workgroups per CU by default; 3 or 4 stages (one workgroup per CU, 2-3 K-tiles in flight)
    // when the grid cannot give a CU two workgroups anyway (small_grid_plan).  GENERAL: the 2-stage tiles and the 3-stage 64 tile.
    // CAP_GEGLU: the fused GEGLU epilogues are built for exactly the (tile, stages, kind) the planner gives a feed-forward GEMM of the training step
    // (B = 16: 5256, 2320, 160 s2 forward, 160 s3 backward) or of SD-2.x @768 (B = 1, 4: 5256, 128 s2, 128 s4 backward, 64 s3 forward, 64 s4 backward);
    // anything else is refused (geglu_refusal) and the caller runs the unfused pair
    {64, 64, 2, 64, 64, CAP_DMA | CAP_STAGED, DMA_FN_GENERAL(256, 64, 64, 2, 2, 2)},
    {64, 64, 3, 64, 64, CAP_DMA | CAP_STAGED | CAP_GEGLU, DMA_FN_GENERAL(256, 64, 64, 2, 2, 3), {}, {}, DMA_GEGLU_F(256, 64, 64, 2, 2, 3, 64)},
    {64, 64, 4, 64, 64, CAP_DMA | CAP_STAGED | CAP_GEGLU, DMA_FN(256, 64, 64, 2, 2, 4, 64), {}, {}, DMA_GEGLU_B(256, 64, 64, 2, 2, 4, 64)},
    // 128x128: 8 waves (wave tile 32x64): ~4 waves/SIMD at 2 workgroups/CU hide the DMA/LDS latency that the 4-wave
    // version of the same tile exposed (measured +5..18 % on every E4T shape, 8192^3: 956 -> 980 TF)
    {128, 64, 2, 128, 128, CAP_DMA | CAP_STAGED | CAP_GEGLU, DMA_FN_GENERAL(512, 128, 128, 4, 2, 2), {}, {}, DMA_GEGLU(512, 128, 128, 4, 2, 2, 64)},
    {128, 64, 3, 128, 128, CAP_DMA | CAP_STAGED, DMA_FN(512, 128, 128, 4, 2, 3, 64)},
    {128, 64, 4, 128, 128, CAP_DMA | CAP_STAGED | CAP_GEGLU, DMA_FN(512, 128, 128, 4, 2, 4, 64), {}, {}, DMA_GEGLU_B(512, 128, 128, 4, 2, 4, 64)},
    {160, 64, 2, 128, 160, CAP_DMA | CAP_STAGED | CAP_TAIL | CAP_GEGLU, DMA_FN_GENERAL(256, 128, 160, 4, 1, 2), {}, {}, DMA_GEGLU_F(256, 128, 160, 4, 1, 2, 64)},
    {160, 64, 3, 128, 160, CAP_DMA | CAP_STAGED | CAP_TAIL | CAP_GEGLU, DMA_FN(256, 128, 160, 4, 1, 3, 64), {}, {}, DMA_GEGLU_B(256, 128, 160, 4, 1, 3, 64)},
    {160, 64, 4, 128, 160, CAP_DMA | CAP_STAGED | CAP_TAIL, DMA_FN(256, 128, 160, 4, 1, 4, 64)},
    // 5256: 256 x 128 with 32-wide K-tiles, 3 x 24 KiB stages = two workgroups per CU; stride-1 convs on conv_strip_kernel where it applies
    {256, 32, 3, 256, 128, CAP_DMA | CAP_GEGLU, DMA_FN(512, 256, 128, 4, 2, 3, 32), {}, {conv_strip_ok, {KERNEL(512, conv_strip_kernel, 2), NO_KERNEL}},
     DMA_GEGLU(512, 256, 128, 4, 2, 3, 32)},
    // 512: 256 x 256 ping-pong; stride-1 convs on gemm_pps_kernel where it applies
    {512, 64, 2, 256, 256, CAP_DMA | CAP_WHOLE_K | CAP_TAIL | CAP_ONE_PER_CU,
     {KERNEL(512, gemm_pp_kernel, 0, false, false), KERNEL(512, gemm_pp_kernel, 0, true, false)},
     {KERNEL(512, gemm_pp_kernel, 1, false, false), KERNEL(512, gemm_pp_kernel, 1, true, false)},
     {KERNEL(512, gemm_pp_kernel, 1, false, true), KERNEL(512, gemm_pp_kernel, 1, true, true)},
     {conv_pps_ok, {KERNEL(512, gemm_pps_kernel, false), KERNEL(512, gemm_pps_kernel, true)}}},
    // 2320: 256 x 320 ping-pong (the GENERAL instantiation exists for GEMMs only)
    {2320, 64, 2, 256, 320, CAP_DMA | CAP_WHOLE_K | CAP_WHOLE_N | CAP_TAIL | CAP_PANELS | CAP_ONE_PER_CU | CAP_GEGLU,
     {KERNEL(512, gemm_pq_kernel, 0, 320, false), KERNEL(512, gemm_pq_kernel, 0, 320, true)}, {KERNEL(512, gemm_pq_kernel, 1, 320, false), NO_KERNEL},
     {}, {}, {KERNEL(512, gemm_pq_geglu_kernel, 320, 1), KERNEL(512, gemm_pq_geglu_kernel, 320, 2)}},
    // the register-staged fallback (operands beyond 4 GB, E4T_GEMM_REGSTAGE), logged as bare "gemm_kernel", GENERAL at run time
    {128, 64, 2, 128, 128, CAP_SPLITK, REG_FN(128, 128, 0), REG_FN(128, 128, 1)},
    {64, 64, 2, 64, 64, CAP_SPLITK, REG_FN(64, 64, 0), REG_FN(64, 64, 1)},
};
// The row of (tile, K-tile width, stages) — stages select only among CAP_STAGED rows — among the LDS-DMA rows or (!dma) the register-staged
// ones; nullptr if there is none.
const Variant* find_variant(int tile, bool kt32, int stages, bool dma = true) {
  for (const Variant& v : kVariants)
    if (!(v.caps & CAP_BUF) == !dma && v.tile == tile && v.kt == (kt32 ? 32 : 64) && (!(v.caps & CAP_STAGED) || v.stages == stages)) return &v;
  return nullptr;
}
const KernelEntry& kernel_of(const Variant& v, bool conv, bool general) { return (conv ? v.conv : v.gemm)[general]; }
// The ONE place that turns a planned row into a kernel entry: launch and launch log both ask it.
const KernelEntry& select_entry(const Variant& v, const GemmArgs& p, bool conv, bool general, int splitk, int batch) {
  if (conv && v.alt.ok && v.alt.k[general].text && v.alt.ok(p, splitk, batch)) return v.alt.k[general];
  if (conv && p.chan_major && v.conv_cm[general].text) return v.conv_cm[general];
  return kernel_of(v, conv, general);
}

// ---- cost model of one launch of the 64 x 64 / 128 x 128 / 128 x 160 DMA tiles (round 4) ---------------------------------------------
// Below a few rounds of workgroups the time of these kernels is set by how many K-tiles a CU keeps in flight, not by the tile's FLOP per
// byte: per 64-wide K-tile a workgroup that is ALONE on its CU needs t1 (its own DMA latency / issue chain: 2 stages expose the whole
// L2 -> LDS latency, 3 - 4 stages hide it but cost the co-resident workgroups their LDS), several co-resident workgroups need tk each
// (the CU's L2 -> LDS bandwidth, ~60 GB/s per CU: 16 / 32 / 36 KiB per K-tile).  A launch costs
//     launch + rounds x (prologue + epilogue) + K-tiles per split x [full rounds x occ x tk + the last, partial round]  (+ the split-K reduce)
// with the workgroups dealt evenly to the CUs.  Constants (us) fitted by least squares to tools/sweep_small_m.py: 75 GEMM / conv shapes
// of the B = 1 / 4 / 16 steps x every (tile, stages, split) = 2900 graph-replayed, cold-operand timings, rms error 8.6 %; the
// argmin is within 6 % of the best measured variant on 72 of them (worst 1.18x), the rules it replaces were 5.8 % slower in total.
struct SmallGridPlan { int tile, stages, splitk; };
struct SmallGridCand { int tile, stages, tm, tn, occ; float t1, tk, epi; bool general_ok; };
SmallGridPlan small_grid_plan(int M, int N, int nkt, bool conv, bool general, int splitk_req, bool wants_colstats, int ncu) {
  static const SmallGridCand cands[] = {
      {64, 3, 64, 64, 3, 0.350f, 0.230f, 0.30f, true},    {64, 4, 64, 64, 2, 0.305f, 0.230f, 0.30f, false},
      {128, 2, 128, 128, 2, 0.875f, 0.544f, 1.08f, true}, {128, 4, 128, 128, 1, 0.596f, 0.544f, 1.08f, false},
      {160, 2, 128, 160, 2, 0.955f, 0.629f, 3.41f, false}, {160, 3, 128, 160, 1, 0.861f, 0.629f, 3.41f, false}};
  static const int splits[] = {1, 2, 3, 4, 6, 8, 12};
  const float launch = 1.6f, pro = 0.945f, red0 = 4.49f, red_bytes_per_us = 4.05e6f, conv_mul = 0.916f, stats_pass = 6.0f;
  SmallGridPlan best = {128, 2, 1};
  float best_t = 1e30f;
  for (const SmallGridCand& c : cands) {
    if (general && !c.general_ok) continue;        // (the GENERAL epilogue is instantiated for these two; the 128 x 160 one is register-bound)
    if (c.tile == 160 && N % 160 != 0) continue;
    for (int sk : splits) {
      if (splitk_req > 0 && sk != 1) continue;     // an explicit split: priced below with the request
      const int s = splitk_req > 0 ? (splitk_req < nkt ? splitk_req : nkt) : sk;
      if (s > 1 && splitk_req <= 0 && (nkt / s < 4 || (double)M * N * s * 4.0 > 256e6)) continue;
      const int kps = cdiv(nkt, s);
      const long long wgs = (long long)cdiv(M, c.tm) * cdiv(N, c.tn) * s;
      const long long per_cu = cdivl(wgs, ncu);
      const long long q = per_cu / c.occ, r = per_cu % c.occ;
      const float full = c.occ > 1 ? c.occ * c.tk : c.t1;
      const float rem = r == 0 ? 0.f : (r == 1 ? c.t1 : (float)r * c.tk);
      float per_kt = (float)q * full + rem;
      if (conv) per_kt *= conv_mul;
      const float rounds = (float)cdivl(per_cu, c.occ);
      float t = launch + rounds * (pro + c.epi) + (float)kps * per_kt;
      if (s > 1) {
        t += red0 + ((float)s * 4.f + 2.f) * (float)M * (float)N / red_bytes_per_us + rounds * c.epi * 0.5f;
        if (wants_colstats) t += stats_pass;       // a split launch leaves no column statistics: the consuming GroupNorm runs its own pass
      }
      if (t < best_t) { best_t = t; best = {c.tile, c.stages, s}; }
    }
  }
  return best;
}

// What launch_gemm() will run for a problem: the ONE place where tiles and split-K are chosen (e4t_gemm_plan / e4t_conv3x3_plan
// export it, so that callers size workspaces and label timings from the launcher's own decision instead of mirroring it).
struct GemmPlan {
  int tile, stages;          // the tile and LDS depth as the public plan reports them
  bool kt32, general_epi, buf_ok;      // kt32: 32-wide K-tiles (codes 5xxx); buf_ok: operands addressable through buffer resources (< 4 GB)
  const Variant* shape;      // the row whose tile shape and capabilities the grid and split-K were planned for
  const Variant* run;        // the row that is launched: `shape`, or the register-staged fallback
  int gx, gy, splitk, ktiles_per_split;
  unsigned a_bytes, a2_bytes, b_bytes;
};

// The planner is a plan under construction, with the problem and what is derived from it once.
struct Planner : GemmPlan {
  const GemmArgs& p;
  const bool conv;
  const int splitk_req, batch, nkt;
  const bool whole_k, dma;             // dma: no E4T_GEMM_REGSTAGE
  int model_splitk;                    // > 0: split-K chosen together with the tile by small_grid_plan
  bool decode_hint(int hint);      // the four stages, in the order plan_gemm() runs them
  void choose_tile();
  void apply_capabilities();
  int choose_splitk() const;
  const Variant* row() {      // the row the choice stands for: a K-tile width the tile has no row for selects nothing, a tile without any row is the default tile
    const Variant* v = find_variant(tile, kt32, stages);
    if (!v && kt32) v = find_variant(tile, false, stages);
    if (!v) { tile = 128; stages = 2; kt32 = false; v = find_variant(128, false, 2); }
    return v;
  }
};

// --- stage 1: a tile hint -> (tile, stages, K-tile width).  64 | 128 | 160 (128 x 160) | 512 (256 x 256 ping-pong) | 2320 (256 x 320
// ping-pong); 3000 / 4000 + tile: 3 / 4 LDS stages of the 64 / 128 / 160 tiles; 5256: 256 x 128 with 32-wide K-tiles.  Anything else (0): automatic.
// The codes of the variants that were measured, rejected and removed stay valid as aliases of the tile that answered them while
// their kernels were kept out of the library: 256 (64-wide 256 x 128), 640 (512 x 128 ping-pong), 1128 / 1160 (persistent streaming kernels),
// 5064 / 5128 (32-wide K-tiles on the 64 / 128 tiles) — and so do the stage / K-tile prefixes on a tile that never had such a row.
bool Planner::decode_hint(int hint) {      // false: the hint names no tile
  static const struct { int hint, alias; } aliases[] = {
      {256, 5256}, {640, 128}, {1128, 128}, {1160, 160}, {5064, 64}, {5128, 128},                           // the retired codes
      {3256, 5256}, {4256, 5256}, {3640, 128}, {4640, 128}, {5640, 128}, {5160, 160}, {5512, 512}};        // a prefix on a tile without such a row
  for (const auto& a : aliases)
    if (hint == a.hint) { hint = a.alias; break; }
  tile = hint; stages = 2; kt32 = false;
  if (hint >= 3000 && hint < 5000) { stages = hint / 1000; tile = hint % 1000; }
  else if (hint >= 5000 && hint < 6000) { kt32 = true; stages = 4; tile = hint % 1000; }
  const Variant* v = find_variant(tile, kt32, stages);
  if (!v) { stages = 2; kt32 = false; return false; }      // choose_tile() starts from the defaults
  if (!(v->caps & CAP_STAGED)) stages = v->stages;
  return true;
}

// --- stage 2: the automatic choice — the measured rules decide WHETHER one of the big tiles runs, then the cost model arbitrates the 64 / 128 /
// 160 tiles, their LDS depth and split-K.  Enters with stages == 2, kt32 == false.  (Round 2's rules: 112.5 vs 110.8 ms per step, profiles/r03_ab/r03c_*.)
void Planner::choose_tile() {
  // fill >= ~1.5 waves of the 256 CUs with 128x128 tiles, else drop to 64x64.  Measured on MI355X (tools/sweep_small.py): 128x128 wins
  // from one full round of the 256 CUs, and already from a quarter round when K is long (3x3 convs at the 16x16 / 8x8 levels) if
  // split-K fills the chip.  (A 64-wide 256 x 128 tile never beat the 2-stage 128 x 128 tile on an E4T shape: DESIGN §2.1.)
  const long long t128 = (long long)cdiv(p.M, 128) * cdiv(p.N, 128) * batch;
  tile = (t128 >= 256 || (nkt >= 32 && t128 >= 64)) ? 128 : 64;
  // every channel count of the SD UNets is a multiple of 160 but 320 / 640 / 960 are not multiples of 128: a 128x160
  // tile has no N padding there (conv 640->640 @32x32: 863 vs 589 TF)
  if (dma && tile == 128 && p.N % 160 == 0 && p.N <= 960 && (long long)cdiv(p.M, 128) * (p.N / 160) * batch >= 128) tile = 160;
  // K-deep shapes whose N is a multiple of 256 and that fill the chip at least twice with 256x256 tiles (the VAE's 256-
  // and 512-channel convs): the ping-pong kernel (conv 512->512 @128^2: 1075 vs 928 TF, 8192^3: 1173 vs 971 TF)
  const long long tpp = (long long)cdiv(p.M, 256) * (p.N / 256) * batch;
  if (dma && tile == 128 && p.N % 256 == 0 && whole_k && nkt >= (conv ? 16 : 20) && tpp >= 512) tile = 512;
  // ... and, with split-K, for the very K-deep shapes of the 16x16 level that give it less than one round of tiles (1280-channel
  // 3x3 convs, the GEGLU input gradient K = 10240): tools/sweep_step_shapes.py, conv 1280->1280 M4096 128 vs 141 us, conv
  // 1280->2560 209 vs 290 us, conv 2560->1280 221 vs 265 us, GEMM 4096x1280x10240 126 vs 138 us; at K = 5120 it loses.  (Round 3:
  // 256..511 tiles are NOT split any more — conv 1280->1280 M16384: 3 splits 545 us, 1 split 482 us, 128 x 160 tile 454 us.)
  if (dma && tile == 128 && p.N % 256 == 0 && whole_k && nkt >= 128 && tpp >= 64 && tpp < 256) tile = 512;
  // one (nearly) full round of ping-pong tiles, K >= 1280: the ViT's qkv projection M4112 N3840 (255 tiles) 44.9 vs 49.5 us,
  // M4096 N3840 42.7 vs 48.3 us
  if (dma && tile == 128 && p.N % 256 == 0 && whole_k && nkt >= 20 && tpp >= 224 && tpp <= 256) tile = 512;
  // (a 512 x 128 variant of the same machine lost to the 128 x 128 tile on the shapes it was built for, 526 vs 588 TF/s: DESIGN §2.1)
  // Round 3 (tools/sweep_ps.py on the step's own shapes, cold operands):
  //  * the 128 x 160 tile also for N > 960 when K is deep and the grid is large — conv 640->1920 M16384 350 vs 378 us, conv
  //    1280->1280 M16384 454 vs 482 (ping-pong) / 492 (128 x 128), GEMM M4096 N5120 K1280 60 vs 64 us; on short K it loses
  //    (M16384 N5120 K640: 145 vs 127 us), and its GELU instantiation is register-bound (M4112 N5120: 107 vs 85 us);
  if (dma && tile == 128 && !general_epi && p.N % 160 == 0 && p.N > 960 && nkt >= 20 &&
      (long long)cdiv(p.M, 128) * (p.N / 160) * batch >= 1024) tile = 160;
  //  * 256 x 128 with 32-wide K-tiles (8 waves, wave tile 64 x 64, three 24-KiB stages = two workgroups per CU; code 5256) for
  //    tall outputs whose N is a multiple of 128: half the B re-reads and 2/3 of the fragment LDS reads of the 128 x 128 tile per
  //    flop.  VAE conv 128->128 @512^2 1449 vs 1744 us, stride-2 conv 455 vs 493, conv_in GEMM M4194304 N128 K32 261 vs 386 (no
  //    padding of K to 64), GEMM M65536 N2560 K320 162 vs 185, M65536 N1280 K320 76 vs 81 us.
  if (dma && tile == 128 && !general_epi && (p.N % 128 == 0 || p.N < 128) &&
      (long long)cdiv(p.M, 256) * cdiv(p.N, 128) * batch >= 768) { tile = 256; kt32 = true; stages = 3; }
  //  * the 256 x 320 ping-pong tile (gemm_pq_kernel, code 2320) wherever N is a multiple of 320 and its rounds of one workgroup per
  //    CU come out full: 0.93 KB of LDS traffic per MFMA against 1.69 KB for the 128 x 160 tile.  Cold-operand sweep
  //    (profiles/r03_sweep_tiles_c.txt): conv 320->320 @64^2 105 vs 127 us (1154 TF/s), 640->640 @64^2 374 vs 458, 1280->1280
  //    M16384 354 vs 439 (1366 TF/s), nearest-x2 + conv 1280->1280 339 vs 472 (1424 TF/s); GEMM M65536 N320 K2560 103 vs 135,
  //    K1280 57 vs 73, K320 26 vs 28; M4096 N10240 K1280 100 vs 112 (ping-pong 256 x 256).  It loses below one round (M16384
  //    N640: 128 tiles) and on the K = 320 GEMMs wider than 320 (epilogue-bound: 83 vs 72 us at N1280).
  //    (Without the 256 x 320 tile: 108.0 vs 106.4 ms per step, profiles/r03_ab/r03h_*.)
  if (dma && batch == 1 && (!general_epi || !conv) && whole_k && p.N % 320 == 0) {
    const long long t320 = (long long)cdiv(p.M, 256) * (p.N / 320);
    const int ncu = device_cu_count();
    const double eff = (double)t320 / (double)(cdivl(t320, ncu) * ncu);
    if (t320 >= ncu && ((nkt >= 20 && eff >= 0.75) || (nkt >= 10 && eff >= 0.99) || (nkt >= 5 && p.N == 320 && eff >= 0.99))) {
      tile = 2320; kt32 = false; stages = 2;
    }
  }
  // (persistent 256 x 160 / 256 x 128 streaming kernels were slower than the tiles above on every shape of the step: DESIGN §2.1)
  // Round 4: the 64 / 128 / 160 tiles, their LDS depth and split-K are arbitrated by a cost model of the launch (small_grid_plan above)
  // instead of the rules that chose among them until round 3; the rules above still decide WHETHER one of the big tiles runs.
  // (The round-3 rules instead of the cost model: C5 B = 1 44.4 vs 39.8 ms, profiles/r04_ab/r04s_*.)
  if (dma && (tile == 64 || tile == 128 || tile == 160) && batch == 1 && !p.reduce_batch && !p.panel_rows) {
    const SmallGridPlan sg = small_grid_plan(p.M, p.N, nkt, conv, general_epi, splitk_req, p.colstats != nullptr, device_cu_count());
    tile = sg.tile; stages = sg.stages; model_splitk = sg.splitk;
  }
}

// --- stage 3: every capability the chosen row lacks for this problem sends it to a narrower tile — 128 x 128, or 128 x 160 where the
// row's own width is a multiple of 160 and N allows it.  Also computes the operand extents (buf_ok).
void Planner::apply_capabilities() {
  auto narrower = [&](const Variant* v) { return v && v->tn % 160 == 0 && p.N % 160 == 0 ? 160 : 128; };
  // epilogues with the exact GELU or a per-row row-bias lookup run the GENERAL instantiation, built for the 2-stage 64 / 128 / 160 tiles (and
  // the 3-stage 64 tile), the 256 x 256 / 256 x 320 (GEMM only) ping-pong kernels; no 32-wide-K kernel has it
  if (general_epi) {
    kt32 = false;
    const Variant* v = find_variant(tile, false, stages);
    if (!(v && (v->caps & CAP_STAGED) && kernel_of(*v, conv, true).text)) { stages = 2; v = find_variant(tile, false, 2); }
    if (!(v && kernel_of(*v, conv, true).text)) tile = narrower(v);
  }
  const Variant* v = row();
  auto fall = [&](int t) { tile = t; v = row(); };
  // E4T_GEMM_REGSTAGE: only the tiles the register-staged kernel is built for
  if (!dma && !find_variant(tile, false, 2, false)) fall(128);
  // row panels: the row that carries them, where the problem meets its other needs
  if (p.panel_rows && !(v->caps & CAP_PANELS))
    for (const Variant& w : kVariants)
      if ((w.caps & CAP_PANELS) && p.N % w.tn == 0 && whole_k && !conv) fall(w.tile);
  // The DMA kernels address their operands through buffer resources (32-bit byte offsets): operands beyond 4 GB fall back to
  // the register-staged kernel.  The ping-pong kernels additionally need whole K-tiles.
  const unsigned long long lim = 0xFFFF0000ull;
  unsigned long long ab, a2b = 0, bb = ((unsigned long long)(p.N - 1) * p.ldb + p.K) * 2;
  if (conv) ab = (unsigned long long)((long long)p.M / ((long long)p.Hout * p.Wout)) * p.Hin * p.Win * p.Cin * 2;   // batch * Hin * Win * Cin
  else {
    const unsigned long long last = p.panel_rows ? (unsigned long long)((p.M - 1) / p.panel_rows) * p.panel_stride + p.panel_off + (p.M - 1) % p.panel_rows : (unsigned long long)(p.M - 1);
    ab = (last * p.lda + p.K1) * 2;
    if (p.A2) a2b = (last * p.lda2 + (p.K - p.K1)) * 2;
  }
  buf_ok = ab < lim && a2b < lim && bb < lim;
  if ((v->caps & CAP_WHOLE_K) && !whole_k) fall(128);
  if ((v->caps & CAP_WHOLE_N) && p.N % v->tn != 0) fall(128);
  a_bytes = (unsigned)(buf_ok ? ab : 0); a2_bytes = (unsigned)(buf_ok ? a2b : 0); b_bytes = (unsigned)(buf_ok ? bb : 0);
  if (!buf_ok && v->tm >= 128) { tile = 128; stages = 2; kt32 = false; }      // the register-staged fallback exists as 128x128 and 64x64 only
}

// --- stage 4: split-K — only when the grid underfills the chip and K is long.
int Planner::choose_splitk() const {
  const Variant& v = *shape;
  int splitk = splitk_req;
  if (!(v.caps & CAP_SPLITK) || p.panel_rows) splitk = 1;
  if (splitk <= 0 && model_splitk > 0 && (v.caps & CAP_STAGED)) splitk = model_splitk;
  if (splitk <= 0) {
    splitk = 1;
    const long long tiles = (long long)gx * gy * batch;
    if (v.caps & CAP_ONE_PER_CU) {
      if (tiles < 256) {
        splitk = (int)(256 / tiles);                 // one 512-thread workgroup per CU: fill one round
        if (splitk > nkt / 16) splitk = nkt / 16;
      }                                              // (a second, partial round is not split: 3 splits of 320 tiles measured 545 vs 482 us)
    } else if (v.tm >= 128 && tiles < 512 && nkt >= 32) {
      // 2 workgroups/CU = 512 slots: aim at one full round (<= 256 tiles) or two (measured, tools/sweep_sk.py: 8x8 convs
      // 80 tiles -> 6 splits -16..19 %, 16x16 convs 320 tiles -> 3 splits -10..17 %), keeping >= 16 K-tiles per split
      splitk = (int)((tiles <= 256 ? 512 : 1024) / tiles);
      if (splitk > 8) splitk = 8;
      if (splitk > nkt / 16) splitk = nkt / 16;
      if (tiles > 256 && nkt < 128) splitk = 1;      // the second round only pays on long K (4096x1280x5120: 3 splits +4 %)
    } else if (v.tm < 128 && tiles < 256 && nkt >= 32) {
      splitk = (int)((512 + tiles - 1) / tiles);
      if (splitk > nkt / 16) splitk = nkt / 16;
    }
    if (splitk < 1) splitk = 1;
  }
  return splitk > nkt ? nkt : splitk;
}

GemmPlan plan_gemm(const GemmArgs& p, bool conv, int tile_hint, int splitk_req, int batch) {
  const bool whole_k = p.K % BK == 0 && (!p.A2 || p.K1 % BK == 0), dma = dma_allowed();
  Planner s = {{}, p, conv, splitk_req, batch, cdiv(p.K, BK), whole_k, dma, 0};
  s.general_epi = (p.flags & E4T_ACT_GELU) || (p.rowbias && p.rows_per_batch % 32 != 0);
  if (!s.decode_hint(tile_hint)) s.choose_tile();
  s.apply_capabilities();
  s.shape = s.row();
  // the register-staged row of the tile (E4T_GEMM_REGSTAGE with row panels keeps the 256 x 320 tile, which has none: the 64 x 64 row, refused at launch)
  const Variant* reg = find_variant(s.tile, false, 2, false);
  s.run = dma && s.buf_ok ? s.shape : reg ? reg : find_variant(64, false, 2, false);
  s.gx = cdiv(p.N, s.shape->tn); s.gy = cdiv(p.M, s.shape->tm);
  s.ktiles_per_split = cdiv(s.nkt, s.choose_splitk());
  s.splitk = cdiv(s.nkt, s.ktiles_per_split);
  return s;
}

// Tail rows (gemm_common.h, gemm_tail): a dense GEMM whose M is a multiple of 128 plus at most 32 rows — the CLIP-ViT's 16 x 257 =
// 4112 token rows — is planned for its first M - r rows; the r tail rows are computed at the end of the same launch.  Returns the plan
// and sets `tail` (0: the ordinary plan over all M rows).  The plan of the M - r rows must be a single pass of one of the LDS-DMA kernels
// that carry the tail code (CAP_TAIL: 128 x 160, 256 x 256 and 256 x 320 tiles): anything else falls back to the plan over all rows.
// (Without the tail stage: README recipe 134.1 vs 133.5 ms, C4 139.6 vs 139.4, headline step equal; profiles/r05_ab.)
GemmPlan plan_gemm_tail(const GemmArgs& p, bool conv, int tile_hint, int splitk_req, int batch, int& tail) {
  tail = 0;
  const int r = p.M % 128;
  if (dma_allowed() && !conv && batch == 1 && !p.reduce_batch && !p.A2 && !p.panel_rows && !p.colstats && splitk_req <= 1 && r > 0 && r <= 32 &&
      p.M - r >= 1024 && p.K % 16 == 0 && p.lda % 8 == 0 && p.ldb % 8 == 0 && (((uintptr_t)p.A | (uintptr_t)p.B) & 15) == 0) {
    GemmArgs q = p;
    q.M = p.M - r;
    const GemmPlan pl = plan_gemm(q, conv, tile_hint, splitk_req, batch);
    if (pl.buf_ok && pl.splitk == 1 && (pl.run->caps & CAP_TAIL)) { tail = r; return pl; }
  }
  return plan_gemm(p, conv, tile_hint, splitk_req, batch);
}

// bf16 C (and residual) with nothing but whole 16-byte groups in every row: what the 8-columns-per-thread epilogues need
bool bf16_rows_aligned16(const GemmArgs& p) {
  return !(p.flags & (E4T_OUT_F32 | E4T_ACCUM | E4T_RES_F32)) && p.N % 8 == 0 && p.ldc % 8 == 0 && ((uintptr_t)p.C & 15) == 0 &&
         (!p.residual || (p.ldr % 8 == 0 && ((uintptr_t)p.residual & 15) == 0));
}

struct ReduceKernel { void (*fn)(GemmArgs, int); const char* text; int cols; };      // cols: columns per thread
// the 8-columns-per-thread kernel when C is bf16 and everything it touches is 16-byte aligned (vec8); the float4 reduction for fp32 C
// with nothing in the epilogue but alpha (and accumulate) and 16-byte aligned rows; else the scalar kernel
const ReduceKernel& reduce_kernel(const GemmArgs& p, bool vec8) {
  static const ReduceKernel k8 = {splitk_reduce8_kernel, "splitk_reduce8_kernel", 8}, k4f = {splitk_reduce4f_kernel, "splitk_reduce4f_kernel", 4},
                            k1 = {splitk_reduce_kernel, "splitk_reduce_kernel", 1};
  const bool f4 = p.ws && (p.flags & E4T_OUT_F32) && !(p.flags & E4T_ACT_GELU) && !p.bias && !p.rowbias && !p.residual && p.N % 4 == 0 && p.ldc % 4 == 0 &&
                  p.strideC % 4 == 0 && (((uintptr_t)p.C | (uintptr_t)p.ws) & 15) == 0;
  return vec8 ? k8 : f4 ? k4f : k1;
}
// (the log line of a launch's reduction is written with the launch's own, before anything is launched)
void log_splitk_reduce(const GemmArgs& p, int nz, int slabs, bool vec8) {
  E4T_LOG_LAUNCH("%s|M%d N%d nz%d|%.0f|0", reduce_kernel(p, vec8).text, p.M, p.N, nz,
                 4.0 * (double)p.M * p.N * slabs + ((p.flags & E4T_OUT_F32) ? 4.0 : 2.0) * (double)p.M * p.N);
}
int launch_splitk_reduce(const GemmArgs& p, int nz, int batch_dim, bool vec8, hipStream_t st) {
  const ReduceKernel& k = reduce_kernel(p, vec8);
  const size_t total = (size_t)p.M * p.N;
  int blocks = (int)((total / k.cols + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k.fn, dim3(blocks, batch_dim), dim3(256), 0, st, p, nz);
  E4T_CHECK_LAUNCH("splitk_reduce_kernel");
  return 0;
}

// ---- fused GEGLU epilogues (E4T_EPI_GEGLU / E4T_EPI_GEGLU_BWD) --------------------------------------------------------------------------
// The flags do not enter the plan: a fused descriptor gets the plan of the plain descriptor of the same M, N, K.  The launch (and the exported
// plan) is refused with E4T_ERR_NO_FUSED unless that plan is ONE pass of a CAP_GEGLU row with the vectorised bf16 epilogue over all rows.
int epi_kind(const GemmArgs& p) { return (p.flags & E4T_EPI_GEGLU) ? EPI_GEGLU : (p.flags & E4T_EPI_GEGLU_BWD) ? EPI_GEGLU_BWD : EPI_PLAIN; }
const char* geglu_refusal(const GemmPlan& pl, const GemmArgs& p, int tail, int batch) {
  const int epi = epi_kind(p);
  if ((p.flags & ~(E4T_EPI_GEGLU | E4T_EPI_GEGLU_BWD)) || ((p.flags & E4T_EPI_GEGLU) && (p.flags & E4T_EPI_GEGLU_BWD))) return "no other epilogue flag combines with it";
  if (p.residual || p.rowbias || p.colstats || p.A2 || p.panel_rows || batch != 1) return "no residual / row bias / column statistics / two-source A / row panels / batch";
  if (epi == EPI_GEGLU_BWD && p.bias) return "the backward kind takes no bias";
  if (p.N % (epi == EPI_GEGLU ? 16 : 8) != 0 || p.ldaux % 8 != 0 || ((uintptr_t)p.aux & 15) != 0) return "the halves of u and the rows of aux must be whole 16-byte groups";
  if (epi == EPI_GEGLU_BWD && (p.ldc < 2 * p.N || p.ldaux < 2 * p.N)) return "du and u are 2 N columns wide";
  if (!(bf16_rows_aligned16(p))) return "the scalar epilogue would run (C rows not 16-byte aligned)";
  if (tail) return "the plan hands tail rows to the tail stage";
  if (pl.splitk > 1 || p.reduce_batch) return "the plan needs split-K";
  if (pl.general_epi) return "the plan needs the GENERAL epilogue";
  if (pl.run != pl.shape) return "the plan runs the register-staged fallback";
  if (!(pl.run->caps & CAP_GEGLU) || !pl.run->geglu[epi - 1].text) return "the planned tile carries no fused GEGLU epilogue";
  if (epi == EPI_GEGLU && p.N % pl.run->tn != 0) return "N is not a multiple of the planned tile's width";
  return nullptr;
}
#define E4T_REFUSE_FUSED(pl, p, tail, batch)                                                                                              \
  do {                                                                                                                                    \
    if (epi_kind(p) != EPI_PLAIN)                                                                                                        \
      if (const char* why = geglu_refusal(pl, p, tail, batch))                                                                            \
        E4T_FAIL(E4T_ERR_NO_FUSED, "gemm: fused GEGLU M=%d N=%d K=%d not run (plan: tile %d, split-K %d): %s", p.M, p.N, p.K, pl.tile, pl.splitk, why); \
  } while (0)

// What a plan becomes at launch time, in ONE place that launch_gemm() and e4t_conv3x3_kernel() both call: the split-K that really runs (the
// automatic choice falls back to one pass when the workspace is missing or short; an explicit one fails with -12), the K-tiles per split, the
// operand extents, the channel-major K order of stride-1 convs and, from those, the kernel entry.  Fills these fields of p and dereferences
// nothing.  Returns the split-K, or a negative error code with the message set.
int resolve_launch(const GemmPlan& pl, GemmArgs& p, bool conv, int epi, size_t ws_bytes, int splitk_req, int batch, const KernelEntry*& entry) {
  int splitk = pl.splitk;
  p.ktiles_per_split = pl.ktiles_per_split;
  p.a_bytes = pl.a_bytes; p.a2_bytes = pl.a2_bytes; p.b_bytes = pl.b_bytes;
  // stride-1 3x3 convs walk K channel-chunk-major (gemm_common.h, cm_step) in every DMA kernel
  // (tap-major K order: 109.7 vs 107.5 ms per step, 2.4-5.2 x the HBM traffic; profiles/r03_ab/r03p_*)
  p.chan_major = conv && pl.buf_ok && p.mode == E4T_CONV_S1 && p.Cin % BK == 0 && p.K == 9 * p.Cin && batch == 1 &&
                 (unsigned long long)p.a_bytes + (unsigned long long)(p.Win + 1) * p.Cin * 2 < 0xFFFF0000ull;
  const bool need_ws = splitk > 1 || p.reduce_batch;
  const size_t need = (size_t)splitk * batch * p.M * p.N * sizeof(float);
  if (need_ws && (p.ws == nullptr || ws_bytes < need)) {
    if (splitk_req > 1 || p.reduce_batch)
      E4T_FAIL(-12, "gemm: split-K=%d batch=%d needs %zu workspace bytes, have %zu", splitk, batch, need, ws_bytes);
    splitk = 1;  // auto mode: fall back to a single pass rather than fail
    p.ktiles_per_split = cdiv(p.K, BK);
  }
  if (!(splitk > 1 || p.reduce_batch)) p.ws = nullptr;
  p.splitk = splitk;
  const KernelEntry& k = epi != EPI_PLAIN ? pl.run->geglu[epi - 1] : select_entry(*pl.run, p, conv, pl.general_epi, splitk, batch);
  if (!k.text) E4T_FAIL(-22, "gemm: no kernel is built for tile %d (%s, GENERAL %d)", pl.tile, conv ? "conv" : "gemm", (int)pl.general_epi);
  entry = &k;
  return splitk;
}

// Everything a launch decides between the plan and the kernel launch, in ONE place that launch_gemm() and e4t_gemm_kernel() both call, so that
// the launch cannot decide anything the query does not see: the fused-GEGLU refusal, the tail rows taken off the tile grid, resolve_launch()
// (split-K that really runs, kernel entry), the store path of write_tile (fast_epi / fast_f32 / scalar / split-K partial), whether column
// statistics are written, the reduce kernel (vec8 and reduce_kernel()) and the row-panel refusal.  Fills p; dereferences nothing.
struct LaunchDecision {
  const KernelEntry* entry;
  const ReduceKernel* reduce;      // nullptr: no reduction follows
  int splitk, nz, m_all, epi, store, stats_written;
  bool vec8;
};
// the branch order of write_tile (gemm_common.h), restated on the host for the query: keep the two together
int store_path(const GemmArgs& p, int epi) {
  return epi != EPI_PLAIN ? E4T_STORE_BF16_STAGED : p.ws ? E4T_STORE_SPLITK_PARTIAL : p.fast_epi ? E4T_STORE_BF16_STAGED : p.fast_f32 ? E4T_STORE_F32_DIRECT : E4T_STORE_SCALAR;
}
int decide_launch(const GemmPlan& pl, GemmArgs& p, bool conv, int tail, size_t ws_bytes, int splitk_req, int batch, LaunchDecision& ld) {
  const Variant& v = *pl.run;
  const int epi = ld.epi = conv ? EPI_PLAIN : epi_kind(p);
  E4T_REFUSE_FUSED(pl, p, tail, batch);
  ld.m_all = p.M;                        // (launch log: the caller's shape)
  if (tail) { p.M -= tail; p.tail_row0 = p.M; p.tail_rows = tail; }      // the tile grid covers [0, M - tail); gemm_tail() the rest
  const int splitk = resolve_launch(pl, p, conv, epi, ws_bytes, splitk_req, batch, ld.entry);
  if (splitk < 0) return splitk;
  ld.splitk = splitk;
  p.group_m = 8;                           // row panels per raster group (swept in round 4: profiles/r04_ab/r04f_*)
  p.fast_epi = bf16_rows_aligned16(p) && p.strideC % 8 == 0;
  p.fast_f32 = (p.flags & E4T_OUT_F32) && !(p.flags & E4T_ACCUM) && !p.rowbias && (!p.residual || (p.flags & E4T_RES_F32)) &&
               (!(p.flags & E4T_ACT_GELU) || pl.general_epi);
  if (p.colstats && (p.ws || !p.fast_epi || p.M % 32 != 0 || batch != 1)) p.colstats = nullptr;   // only the bf16 single-pass epilogue produces them
  ld.stats_written = p.colstats != nullptr && (v.caps & CAP_COLSTATS);
  // split-K / batch reduction: 8 columns per thread when bias, row bias and workspace are 16-byte aligned too
  ld.vec8 = p.ws && bf16_rows_aligned16(p) && p.strideC % 8 == 0 &&
            (!p.bias || (((uintptr_t)p.bias & 15) == 0 && p.strideBias % 4 == 0)) &&
            (!p.rowbias || (((uintptr_t)p.rowbias & 15) == 0 && p.ldrb % 4 == 0)) && ((uintptr_t)p.ws & 15) == 0;
  ld.nz = p.reduce_batch ? splitk * batch : splitk;
  ld.reduce = p.ws ? &reduce_kernel(p, ld.vec8) : nullptr;
  ld.store = store_path(p, epi);
  if (p.panel_rows && !((v.caps & CAP_PANELS) && splitk == 1 && !p.ws))
    E4T_FAIL(-22, "gemm: row panels need the 256 x 320 ping-pong tile (N %% 320 == 0, K %% 64 == 0, no split-K); the plan chose tile %d", pl.tile);
  return splitk;
}

int launch_gemm(GemmArgs p, bool conv, int tile_hint, size_t ws_bytes, int splitk_req, int batch, hipStream_t st) {
  int tail = 0;
  const GemmPlan pl = plan_gemm_tail(p, conv, tile_hint, splitk_req, batch, tail);
  LaunchDecision ld = {};
  const int splitk = decide_launch(pl, p, conv, tail, ws_bytes, splitk_req, batch, ld);
  if (splitk < 0) return splitk;
  const KernelEntry& k = *ld.entry;
  const int epi = ld.epi, m_all = ld.m_all, nz = ld.nz, stats_written = ld.stats_written;
  const bool vec8 = ld.vec8;
  if (e4t_launch_log_enabled()) {
    // algorithmic bytes: every operand element once (conv: the input map once, not once per tap), the output once
    const double osz = (p.flags & E4T_OUT_F32) ? 4.0 : 2.0;
    const double a_el = conv ? (double)(p.M / ((long long)p.Hout * p.Wout)) * p.Hin * p.Win * p.Cin : (double)p.M * p.K * batch;
    double by = 2.0 * a_el + 2.0 * (double)p.N * p.K * (p.strideB || batch == 1 ? batch : 1) + osz * (double)p.M * p.N * (p.reduce_batch ? 1 : batch);
    if (p.residual) by += ((p.flags & E4T_RES_F32) ? 4.0 : 2.0) * (double)p.M * p.N;
    if (p.flags & E4T_ACCUM) by += osz * (double)p.M * p.N;
    if (conv) E4T_LOG_LAUNCH("%s|conv mode%d %dx%d->%dx%d Cin%d Cout%d M%d splitk%d|%.0f|%.0f", k.text, p.mode, p.Hin, p.Win, p.Hout, p.Wout, p.Cin, p.N,
                             p.M, splitk, by, 2.0 * p.M * p.N * (double)p.K);
    else if (epi != EPI_PLAIN)      // u written + h written | u read + du written (2 N columns each); dh is never stored
      E4T_LOG_LAUNCH("%s|%s M%d N%d K%d batch%d splitk%d flags%d|%.0f|%.0f", k.text, epi == EPI_GEGLU ? "gemm_geglu" : "gemm_geglu_bwd", m_all, p.N, p.K, batch, splitk,
                     p.flags, 2.0 * a_el + 2.0 * (double)p.N * p.K + (p.bias ? 4.0 * p.N : 0.0) + (epi == EPI_GEGLU ? 3.0 : 8.0) * (double)p.M * p.N, 2.0 * m_all * p.N * (double)p.K);
    else E4T_LOG_LAUNCH("%s|gemm M%d N%d K%d batch%d splitk%d flags%d|%.0f|%.0f", k.text, m_all, p.N, p.K, batch, splitk, p.flags,
                        by + (double)tail * (2.0 * p.K + (osz + (p.residual ? ((p.flags & E4T_RES_F32) ? 4.0 : 2.0) : 0.0)) * p.N), 2.0 * m_all * p.N * (double)p.K * batch);
    if (p.ws) log_splitk_reduce(p, nz, splitk * batch, vec8);
  }
  hipLaunchKernelGGL(k.fn, dim3(pl.gx, pl.gy, splitk * batch), dim3(k.threads), 0, st, p);
  E4T_CHECK_LAUNCH("gemm_kernel");
  if (const int rc = p.ws ? launch_splitk_reduce(p, nz, p.reduce_batch ? 1 : batch, vec8, st) : 0; rc < 0) return rc;
  return stats_written;
}

}  // namespace

namespace {

void fill_gemm_args(const e4t_gemm_desc* d, GemmArgs& p) {
  memset(&p, 0, sizeof(p));
  p.zslab = -1;
  p.A = (const bf16_t*)d->A; p.A2 = (const bf16_t*)d->A2; p.K1 = d->A2 ? d->K1 : d->K; p.lda = d->lda; p.lda2 = d->lda2;
  p.B = (const bf16_t*)d->B; p.ldb = d->ldb; p.C = d->C; p.ldc = d->ldc; p.bias = d->bias; p.residual = d->residual; p.ldr = d->ldr;
  p.rowbias = d->rowbias; p.rows_per_batch = d->rows_per_batch > 0 ? d->rows_per_batch : 1; p.ldrb = d->ldrb > 0 ? d->ldrb : d->N;
  p.M = d->M; p.N = d->N; p.K = d->K; p.alpha = d->alpha; p.flags = d->flags; p.ws = (float*)d->workspace;
  p.strideA = d->strideA; p.strideB = d->strideB; p.strideC = d->strideC; p.strideBias = d->strideBias;
  p.reduce_batch = (d->flags & E4T_REDUCE_BATCH) ? 1 : 0;
  p.colstats = d->colstats;
  p.panel_rows = d->panel_rows; p.panel_stride = d->panel_stride; p.panel_off = d->panel_off;
  p.aux = d->aux; p.ldaux = d->ldaux;
}

// the geometry a conv descriptor must have, for the launch and for the kernel query alike
int check_conv_geometry(const e4t_conv_desc* d) {
  const int Cin = d->Cin, Cout = d->Cout, Hin = d->Hin, Win = d->Win, Hout = d->Hout, Wout = d->Wout, mode = d->mode;
  E4T_REQUIRE(Cin % BK == 0, "conv3x3: Cin=%d must be a multiple of 64 (pad the input channels)", Cin);
  E4T_REQUIRE(mode >= E4T_CONV_S1 && mode <= E4T_CONV_S2A, "conv3x3: bad mode %d", mode);
  E4T_REQUIRE(d->B > 0 && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0 && Cout > 0, "conv3x3: bad geometry");
  if (mode == E4T_CONV_S1) E4T_REQUIRE(Hout == Hin && Wout == Win, "conv3x3 S1: output must equal input size");
  if (mode == E4T_CONV_S2) E4T_REQUIRE(Hout == (Hin - 1) / 2 + 1 && Wout == (Win - 1) / 2 + 1, "conv3x3 S2: bad output size");
  if (mode == E4T_CONV_UP2) E4T_REQUIRE(Hout == 2 * Hin && Wout == 2 * Win, "conv3x3 UP2: output must be 2x input");
  if (mode == E4T_CONV_S2T) E4T_REQUIRE(Hin == (Hout - 1) / 2 + 1 && Win == (Wout - 1) / 2 + 1, "conv3x3 S2T: bad sizes");
  if (mode == E4T_CONV_S2A) E4T_REQUIRE(Hout == (Hin - 2) / 2 + 1 && Wout == (Win - 2) / 2 + 1, "conv3x3 S2A: bad output size");
  return 0;
}

void fill_conv_args(const e4t_conv_desc* d, GemmArgs& p) {
  const int Cin = d->Cin, Cout = d->Cout;
  memset(&p, 0, sizeof(p));
  p.zslab = -1;
  p.A = (const bf16_t*)d->X; p.K1 = 9 * Cin; p.Hin = d->Hin; p.Win = d->Win; p.Cin = Cin; p.Hout = d->Hout; p.Wout = d->Wout;
  p.mode = d->mode; p.B = (const bf16_t*)d->W; p.ldb = 9 * Cin; p.C = d->Y; p.ldc = Cout; p.bias = d->bias;
  p.residual = d->residual; p.ldr = Cout; p.rowbias = d->rowbias; p.rows_per_batch = d->Hout * d->Wout; p.ldrb = d->ldrb > 0 ? d->ldrb : Cout;
  p.M = d->B * d->Hout * d->Wout; p.N = Cout; p.K = 9 * Cin; p.alpha = 1.f; p.flags = d->flags; p.ws = (float*)d->workspace;
  p.colstats = d->colstats;
}

// split count of the TN (weight-gradient) kernel: few output tiles, very long K -> fill the 512 workgroup slots by splitting K
int tn_splitk(int M, int N, int K, int req) {
  const int nkt = cdiv(K, BK);
  const long long tiles = (long long)cdiv(N, 128) * cdiv(M, 128);
  int splitk = req;
  if (splitk <= 0) {
    splitk = (int)(512 / tiles);
    if (splitk > 32) splitk = 32;
    if (splitk > nkt / 16) splitk = nkt / 16;
    if (splitk < 1) splitk = 1;
  }
  if (splitk > nkt) splitk = nkt;
  return cdiv(nkt, cdiv(nkt, splitk));
}

// 5000 + tile for 32-wide K-tiles; `stages` only where it is a choice (the 64-wide 64 / 128 / 160 tiles)
void export_plan(const GemmPlan& pl, const GemmArgs& p, int batch, e4t_gemm_plan_t* out, int tail = 0) {
  out->tile = pl.kt32 ? 5000 + pl.tile : pl.tile; out->tile_m = pl.shape->tm; out->tile_n = pl.shape->tn; out->splitk = pl.splitk;
  out->workspace_bytes = (pl.splitk > 1 || p.reduce_batch) ? (size_t)pl.splitk * batch * p.M * p.N * sizeof(float) : 0;
  out->tail_rows = tail; out->stages = (!pl.kt32 && (pl.shape->caps & CAP_STAGED)) ? pl.stages : 0;
}

}  // namespace

extern "C" int e4t_gemm_plan(const e4t_gemm_desc* d, e4t_gemm_plan_t* out) {
  E4T_REQUIRE(d && out && d->M > 0 && d->N > 0 && d->K > 0, "gemm_plan: bad arguments");
  GemmArgs p;
  fill_gemm_args(d, p);
  const int batch = d->batch > 0 ? d->batch : 1;
  int tail = 0;
  const GemmPlan pl = plan_gemm_tail(p, false, d->tile, d->splitk, batch, tail);
  export_plan(pl, p, batch, out, tail);      // (no workspace with tail rows: their plan is a single pass)
  E4T_REFUSE_FUSED(pl, p, tail, batch);      // a fused descriptor: the plain plan is exported either way; the code says whether the fused kernel will run
  return 0;
}

extern "C" int e4t_conv3x3_plan(const e4t_conv_desc* d, e4t_gemm_plan_t* out) {
  E4T_REQUIRE(d && out && d->B > 0 && d->Hout > 0 && d->Wout > 0 && d->Cin > 0 && d->Cout > 0, "conv3x3_plan: bad arguments");
  GemmArgs p;
  fill_conv_args(d, p);
  export_plan(plan_gemm(p, true, d->tile, d->splitk, 1), p, 1, out);
  return 0;
}

extern "C" int e4t_gemm_tn_plan(const e4t_gemm_desc* d, e4t_gemm_plan_t* out) {
  E4T_REQUIRE(d && out && d->M > 0 && d->N > 0 && d->K > 0, "gemm_tn_plan: bad arguments");
  out->tile = 128; out->tile_m = out->tile_n = 128; out->tail_rows = out->stages = 0;
  out->splitk = tn_splitk(d->M, d->N, d->K, d->splitk);
  out->workspace_bytes = out->splitk > 1 ? (size_t)out->splitk * d->M * d->N * sizeof(float) : 0;
  return 0;
}

namespace {

// the arguments e4t_gemm_nt accepts, for the launch and for the kernel query alike
int check_gemm_nt_args(const e4t_gemm_desc* d) {
  E4T_REQUIRE(d && d->A && d->B && d->C, "gemm_nt: null operand");
  E4T_REQUIRE(d->M > 0 && d->N > 0 && d->K > 0, "gemm_nt: bad shape M=%d N=%d K=%d", d->M, d->N, d->K);
  E4T_REQUIRE(d->K % 8 == 0 && d->lda % 8 == 0 && d->ldb % 8 == 0, "gemm_nt: K, lda, ldb must be multiples of 8 (16-B rows)");
  E4T_REQUIRE(((uintptr_t)d->A & 15) == 0 && ((uintptr_t)d->B & 15) == 0, "gemm_nt: A/B must be 16-B aligned");
  if (d->A2) {
    E4T_REQUIRE(d->K1 % BK == 0 && d->K1 > 0 && d->K1 < d->K && d->lda2 % 8 == 0 && ((uintptr_t)d->A2 & 15) == 0,
                "gemm_nt: two-source A needs K1 %% 64 == 0, 0 < K1 < K");
  }
  E4T_REQUIRE(!d->rowbias || d->rows_per_batch > 0, "gemm_nt: rowbias needs rows_per_batch");
  const int batch = d->batch > 0 ? d->batch : 1;
  E4T_REQUIRE(batch == 1 || (d->strideA % 8 == 0 && d->strideB % 8 == 0), "gemm_nt: batch strides must keep 16-B alignment");
  E4T_REQUIRE(!(d->flags & E4T_REDUCE_BATCH) || !d->A2, "gemm_nt: reduce-batch with two-source A unsupported");
  if (d->panel_rows) {
    E4T_REQUIRE(d->panel_rows > 0 && d->panel_rows % 256 == 0 && d->panel_stride >= d->panel_rows && d->panel_off >= 0 && d->M % d->panel_rows == 0,
                "gemm_nt: row panels need panel_rows %% 256 == 0, panel_stride >= panel_rows, M %% panel_rows == 0");
    E4T_REQUIRE(batch == 1 && !d->rowbias && !d->colstats && !d->A2 && !(d->flags & (E4T_ACCUM | E4T_REDUCE_BATCH)) && d->splitk <= 1,
                "gemm_nt: row panels do not combine with batch / row bias / column statistics / two-source A / accumulate / split-K");
  }
  E4T_REQUIRE(!(d->flags & (E4T_EPI_GEGLU | E4T_EPI_GEGLU_BWD)) || d->aux, "gemm_nt: the fused GEGLU epilogues need aux (h out / u in)");
  return 0;
}

// What e4t_gemm_tn decides before its launch, in ONE place that the launch and e4t_gemm_tn_kernel() both call: argument checks, operand extents, the
// split-K that really runs (the automatic choice falls back to one pass without its workspace, an explicit one fails with -12), the store path.
// Fills p and dereferences nothing.  Returns the split-K, or a negative error code with the message set.
int resolve_tn(const e4t_gemm_desc* d, GemmArgs& p) {
  E4T_REQUIRE(d && d->A && d->B && d->C, "gemm_tn: null operand");
  E4T_REQUIRE(d->M > 0 && d->N > 0 && d->K > 0 && d->batch <= 1 && !d->A2 && !d->rowbias, "gemm_tn: bad / unsupported arguments");
  E4T_REQUIRE(!(d->flags & (E4T_ACT_GELU | E4T_EPI_GEGLU | E4T_EPI_GEGLU_BWD)), "gemm_tn: the GELU / GEGLU epilogues are not built for the TN kernel");
  E4T_REQUIRE(d->M % 8 == 0 && d->N % 8 == 0 && d->lda % 8 == 0 && d->ldb % 8 == 0 && ((uintptr_t)d->A & 15) == 0 && ((uintptr_t)d->B & 15) == 0,
              "gemm_tn: M, N, lda, ldb must be multiples of 8 and the operands 16-byte aligned");
  // (not fill_gemm_args: the fields the TN kernel does not support — lda2, strides, row panels, ... — stay zero whatever the caller left there)
  memset(&p, 0, sizeof(p));
  p.zslab = -1;
  p.A = (const bf16_t*)d->A; p.lda = d->lda; p.B = (const bf16_t*)d->B; p.ldb = d->ldb;
  p.C = d->C; p.ldc = d->ldc; p.bias = d->bias; p.residual = d->residual; p.ldr = d->ldr;
  p.M = d->M; p.N = d->N; p.K = d->K; p.K1 = d->K; p.alpha = d->alpha; p.flags = d->flags & ~E4T_REDUCE_BATCH;
  p.rows_per_batch = 1; p.ldrb = d->N;
  p.ws = (float*)d->workspace;
  const int nkt = cdiv(p.K, BK);
  {   // operand extents for the buffer resources (32-bit byte offsets)
    const unsigned long long ab = ((unsigned long long)(p.K - 1) * p.lda + p.M) * 2, bb = ((unsigned long long)(p.K - 1) * p.ldb + p.N) * 2;
    E4T_REQUIRE(ab < 0xFFFF0000ull && bb < 0xFFFF0000ull, "gemm_tn: operands beyond 4 GB are not supported");
    p.a_bytes = (unsigned)ab; p.b_bytes = (unsigned)bb;
  }
  int splitk = tn_splitk(p.M, p.N, p.K, d->splitk);
  p.ktiles_per_split = cdiv(nkt, splitk);
  const size_t need = (size_t)splitk * p.M * p.N * sizeof(float);
  if (splitk > 1 && (p.ws == nullptr || d->workspace_bytes < need)) {
    if (d->splitk > 1) E4T_FAIL(-12, "gemm_tn: split-K=%d needs %zu workspace bytes, have %zu", splitk, need, d->workspace_bytes);
    splitk = 1;
    p.ktiles_per_split = nkt;
  }
  if (splitk <= 1) p.ws = nullptr;
  p.splitk = splitk;
  p.group_m = 8;
  p.xcd3 = splitk > 1;                     // (2-D raster: gemm_tn M960 N320 K65536 90.6 vs 67.4 us)
  p.fast_epi = bf16_rows_aligned16(p);
  return splitk;
}

void export_kernel(const char* symbol, const ReduceKernel* reduce, int splitk, int tail, int store, int stats, e4t_gemm_kernel_t* out) {
  out->symbol = symbol; out->reduce = reduce ? reduce->text : nullptr; out->splitk = splitk; out->tail_rows = tail; out->store = store; out->colstats = stats;
}

}  // namespace

extern "C" int e4t_gemm_nt(const e4t_gemm_desc* d, e4t_stream stream) {
  if (const int rc = check_gemm_nt_args(d); rc < 0) return rc;
  GemmArgs p;
  fill_gemm_args(d, p);
  return launch_gemm(p, false, d->tile, d->workspace_bytes, d->splitk, d->batch > 0 ? d->batch : 1, (hipStream_t)stream);
}

extern "C" int e4t_gemm_kernel(const e4t_gemm_desc* d, e4t_gemm_kernel_t* out) {
  E4T_REQUIRE(out, "gemm_kernel: bad arguments");
  if (const int rc = check_gemm_nt_args(d); rc < 0) return rc;
  GemmArgs p;
  fill_gemm_args(d, p);
  const int batch = d->batch > 0 ? d->batch : 1;
  int tail = 0;
  const GemmPlan pl = plan_gemm_tail(p, false, d->tile, d->splitk, batch, tail);
  LaunchDecision ld = {};
  const int sk = decide_launch(pl, p, false, tail, d->workspace_bytes, d->splitk, batch, ld);
  if (sk < 0) return sk;
  export_kernel(ld.entry->text, ld.reduce, sk, tail, ld.store, ld.stats_written, out);
  return 0;
}

extern "C" int e4t_gemm_tn(const e4t_gemm_desc* d, e4t_stream stream) {
  GemmArgs p;
  const int splitk = resolve_tn(d, p);
  if (splitk < 0) return splitk;
  const int gx = cdiv(p.N, 128), gy = cdiv(p.M, 128);
  hipStream_t st = (hipStream_t)stream;
  if (e4t_launch_log_enabled()) {
    const double osz = (p.flags & E4T_OUT_F32) ? 4.0 : 2.0;
    E4T_LOG_LAUNCH("gemm_tn_kernel|gemm_tn M%d N%d K%d splitk%d flags%d|%.0f|%.0f", p.M, p.N, p.K, splitk, p.flags,
                   2.0 * (double)p.K * (p.M + p.N) + osz * (double)p.M * p.N * ((p.flags & E4T_ACCUM) ? 2 : 1), 2.0 * p.M * p.N * (double)p.K);
    if (p.ws) log_splitk_reduce(p, splitk, splitk, false);
  }
  hipLaunchKernelGGL(gemm_tn_kernel, dim3(gx, gy, splitk), dim3(512), 0, st, p);
  E4T_CHECK_LAUNCH("gemm_tn_kernel");
  return p.ws ? launch_splitk_reduce(p, splitk, 1, false, st) : 0;
}

extern "C" int e4t_gemm_tn_kernel(const e4t_gemm_desc* d, e4t_gemm_kernel_t* out) {
  E4T_REQUIRE(out, "gemm_tn_kernel: bad arguments");
  GemmArgs p;
  const int splitk = resolve_tn(d, p);
  if (splitk < 0) return splitk;
  export_kernel("gemm_tn_kernel", p.ws ? &reduce_kernel(p, false) : nullptr, splitk, 0, store_path(p, EPI_PLAIN), 0, out);
  return 0;
}

extern "C" int e4t_conv3x3(const e4t_conv_desc* d, e4t_stream stream) {
  E4T_REQUIRE(d && d->X && d->W && d->Y, "conv3x3: null operand");
  if (const int rc = check_conv_geometry(d); rc < 0) return rc;
  GemmArgs p;
  fill_conv_args(d, p);
  return launch_gemm(p, true, d->tile, d->workspace_bytes, d->splitk, 1, (hipStream_t)stream);
}

extern "C" int e4t_conv3x3_kernel(const e4t_conv_desc* d, const char** symbol, int* splitk) {
  E4T_REQUIRE(d && symbol && splitk, "conv3x3_kernel: bad arguments");
  if (const int rc = check_conv_geometry(d); rc < 0) return rc;
  GemmArgs p;
  fill_conv_args(d, p);
  int tail = 0;
  const GemmPlan pl = plan_gemm_tail(p, true, d->tile, d->splitk, 1, tail);
  const KernelEntry* entry = nullptr;
  const int sk = resolve_launch(pl, p, true, EPI_PLAIN, d->workspace_bytes, d->splitk, 1, entry);
  if (sk < 0) return sk;
  *symbol = entry->text;
  *splitk = sk;
  return 0;
}
