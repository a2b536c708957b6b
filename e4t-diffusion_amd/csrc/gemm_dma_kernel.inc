// Body of gemm_dma_kernel / gemm_dma_geglu_kernel (gemm.hip), included once into each: the two __global__ templates differ only in the names
// they bind — BM, BN, WGM, WGN, MODE, NSTAGE, GENERAL, KT, EPI (template parameters or constants of the including kernel) — so the plain kernels
// keep their symbols and, not being routed through a shared device function, their code.  `p` is the kernel's GemmArgs.
#ifdef DMA_TRACE
  const int dt_lin = blockIdx.y * gridDim.x + blockIdx.x;
  const int dt_wg = dt_lin >> 3;
  const bool dt_on = (threadIdx.x == 0) && (dt_lin & 7) == 0 && dt_wg < 128 && blockIdx.z == 0;
  DT(0);
#endif
  constexpr int WM = BM / WGM, WN = BN / WGN;
  constexpr int FM = WM / 32, FN = WN / 32;
  constexpr int NW = WGM * WGN;                       // waves per workgroup (4 or 8)
  constexpr int SL = KT / 8;                          // 16-byte slots per LDS row
  constexpr int RPP = 512 / KT;                       // rows per 1-KiB DMA piece (8 or 16)
  constexpr int NA = BM / RPP / NW, NB = (BN / RPP + NW - 1) / NW;   // pieces per wave per K-tile (B: last wave may own fewer)
  constexpr int LOOK = NSTAGE - 1;                    // K-tiles in flight
  constexpr int TILE = (BM + BN) * KT;          // elements per LDS buffer
  static_assert(NA >= 1 && NB >= 1 && (NW == 4 || NW == 8) && (NSTAGE >= 2 && NSTAGE <= 4), "bad tile configuration");
  constexpr bool RAGGED_B = (BN / RPP) % NW != 0;     // the last wave(s) own fewer B pieces: their counted waits use their own count
  static_assert(!RAGGED_B || NB <= 3, "counted vmcnt: per-wave piece counts are enumerated up to 3 B pieces");
  static_assert((KT == 64 || KT == 32) && BM % (RPP * NW) == 0, "bad K-tile width");

  __shared__ __attribute__((aligned(16))) bf16_t smem[NSTAGE * TILE];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (an SGPR: the DMA destinations are wave-uniform)
  const int wm = wave / WGN, wn = wave % WGN;
  // B pieces this wave issues per K-tile (wave-uniform): NB, or fewer in the last wave(s) of a ragged split
  const int nbw = RAGGED_B ? min(NB, max(0, BN / RPP - wave * NB)) : NB;
  int tile_x, tile_y;
  xcd_tile(tile_x, tile_y, p.group_m);
  const int m0 = tile_y * BM, n0 = tile_x * BN;

  const KRange kr = batch_entry<KT>(p, (p.K + KT - 1) / KT);          // (the launcher counts 64-wide tiles)
  const int kt_begin = kr.begin, kt_end = kr.end;

  // Operands are addressed through buffer resources (buffer_load ... lds): a 32-bit per-lane byte offset that changes only
  // when the tile starts a new region — the first tile, a new 3x3 tap (conv), the switch to the second concat source
  // (dense), the ragged last tile — plus a wave-uniform SGPR offset that walks K (+128 B per K-tile).  Issuing a tile costs
  // no VALU at all (a per-tile 64-bit address recomputation cost ~1.2k issue cycles per wave, carried 64-bit pointers still
  // 3 VALU each), and out-of-range rows / conv padding / K tails carry an out-of-range offset: the hardware returns zeros.
  const bool cm = MODE != 0 && p.chan_major;          // channel-chunk-major K order (gemm_common.h, cm_step)
  const __amdgpu_buffer_rsrc_t rs_a = cm ? cm_rsrc(p) : __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, (int)p.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_a2 = __builtin_amdgcn_make_buffer_rsrc((void*)(p.A2 ? p.A2 : p.A), 0, (int)(p.A2 ? p.a2_bytes : p.a_bytes), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc((void*)p.B, 0, (int)p.b_bytes, 0x00020000);
  const int lrow = lane / SL, lslot = lane % SL;   // position of this lane inside a 1-KiB piece

  // rows this lane feeds: piece q = wave*NA + i covers tile rows q*8 .. q*8+7
  long long a_base[NA];
  int a_oy[NA], a_ox[NA], a_kc[NA];
  bool a_ok[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int r = (wave * NA + i) * RPP + lrow;
    const int gr = m0 + r;
    a_ok[i] = gr < p.M;
    a_kc[i] = (lslot ^ swz_slot<KT>(r)) * 8;       // logical k offset (elements) this lane fetches for that row
    if (MODE == 0) {
      a_base[i] = (long long)gr; a_oy[i] = a_ox[i] = 0;
    } else {
      out_pixel(p, gr, a_base[i], a_oy[i], a_ox[i]);
    }
  }
  unsigned b_row[NB];
  int b_kc[NB];
  bool b_ok[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int r = (wave * NB + i) * RPP + lrow;
    const int gn = EPI == EPI_GEGLU ? geglu_col<WN>(n0, r, p.N) : n0 + r;
    b_ok[i] = gn < p.N && r < BN;
    b_kc[i] = (lslot ^ swz_slot<KT>(r)) * 8;
    b_row[i] = (unsigned)(((size_t)(b_ok[i] ? gn : 0) * p.ldb + b_kc[i]) * 2);
  }

  unsigned a_vo[NA], b_vo[NB];
  int a_so = 0, b_so = 0;          // wave-uniform byte offsets along K
  bool a_second = false;           // reading the second concat source
  auto place_a = [&](int k0) {
    if (MODE == 0) {
      int ld = p.lda, koff = k0;      // written out: profiles/gemm_addressing_isa.txt
      a_second = k0 >= p.K1;
      if (a_second) { ld = p.lda2; koff = k0 - p.K1; }
      a_so = __builtin_amdgcn_readfirstlane(koff * 2);          // (wave-uniform by construction; keeps the offset in an SGPR for the compiler)
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const bool ok = a_ok[i] && (k0 + a_kc[i] < p.K);
        a_vo[i] = ok ? (unsigned)((a_base[i] * ld + a_kc[i]) * 2) : OOB;
      }
    } else {
      const int tap = k0 / p.Cin;
      const int ci0 = k0 - tap * p.Cin;
      const int ky = tap / 3, kx = tap - ky * 3;
      a_so = __builtin_amdgcn_readfirstlane(ci0 * 2);
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
        } else if (p.mode == E4T_CONV_UP2) {
          iy = a_oy[i] + ky - 1; ix = a_ox[i] + kx - 1;
          ok = ok && iy >= 0 && iy < 2 * p.Hin && ix >= 0 && ix < 2 * p.Win;
          iy >>= 1; ix >>= 1;
        } else if (p.mode == E4T_CONV_S2A) {
          iy = 2 * a_oy[i] + ky; ix = 2 * a_ox[i] + kx;
          ok = ok && iy < p.Hin && ix < p.Win;
        } else {
          const int sy = a_oy[i] + ky - 1, sx = a_ox[i] + kx - 1;
          ok = ok && sy >= 0 && sx >= 0 && !(sy & 1) && !(sx & 1);
          iy = sy >> 1; ix = sx >> 1;
          ok = ok && iy < p.Hin && ix < p.Win;
        }
        a_vo[i] = ok ? (unsigned)(((a_base[i] + (long long)iy * p.Win + ix) * p.Cin + a_kc[i]) * 2) : OOB;
      }
    }
  };
  auto place_b = [&](int k0) {
    b_so = k0 * 2;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const bool ok = b_ok[i] && (k0 + b_kc[i] < p.K);
      b_vo[i] = ok ? b_row[i] : OOB;
    }
  };
  if (cm) {                        // a_vo = the output position's own pixel (all taps), a_oy = inverted 9-bit tap validity mask
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      a_vo[i] = cm_center(p, a_base[i], a_oy[i], a_ox[i], a_kc[i]);
      a_oy[i] = cm_inv_mask(p, a_ok[i], a_oy[i], a_ox[i]);
    }
  }
  CmWalk wk;                       // cm: (tap, chunk) of the next K-tile to issue
  wk.init(kt_begin, KT);
  const int cm_table = cm ? cm_tap_table(p, lane) : 0;
  auto issue_tile = [&](int kt, bf16_t* buf) __attribute__((always_inline)) {
    const int k0 = kt * KT;
    bf16_t* As = buf;
    bf16_t* Bs = buf + BM * KT;
    if (cm) {                      // whole K-tiles only (Cin % KT == 0): no ragged tile; tiles are issued in increasing kt
      if (kt == kt_begin) place_b(k0);
      const int aso = cm_a_so(cm_table, wk), bso = cm_b_so(p, wk);
#pragma unroll
      for (int i = 0; i < NA; ++i)
        buf_dma16(rs_a, cm_row_off(a_vo[i], a_oy[i], wk), aso, As + (wave * NA + i) * 512);
#pragma unroll
      for (int i = 0; i < NB; ++i)
        if ((BN / RPP) % NW == 0 || wave * NB + i < BN / RPP)
          buf_dma16(rs_b, b_vo[i], bso, Bs + (wave * NB + i) * 512);
      wk.next(KT);
      return;
    }
    const bool ragged = k0 + KT > p.K;                                      // wave-uniform conditions
    const bool fresh_a = kt == kt_begin || ragged || (MODE == 0 ? k0 == p.K1 : (k0 % p.Cin) == 0);
    if (fresh_a) place_a(k0);
    else a_so += KT * 2;
    if (kt == kt_begin || ragged) place_b(k0);
    else b_so += KT * 2;
#pragma unroll
    for (int i = 0; i < NA; ++i)
      buf_dma16(a_second ? rs_a2 : rs_a, a_vo[i], a_so, As + (wave * NA + i) * 512);
#pragma unroll
    for (int i = 0; i < NB; ++i)
      if ((BN / RPP) % NW == 0 || wave * NB + i < BN / RPP)
        buf_dma16(rs_b, b_vo[i], b_so, Bs + (wave * NB + i) * 512);
  };

  f32x16 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int frow = lane & 31, fhi = lane >> 5;
  // fragment offsets inside a stage (elements), one per (fragment, k-step): computed once; the stage base is a
  // compile-time constant of the unrolled loop below, so every ds_read_b128 is "vgpr + immediate"
  int a_off[FM][KT / 16], b_off[FN][KT / 16];
#pragma unroll
  for (int ks = 0; ks < KT / 16; ++ks) {
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int r = wm * WM + i * 32 + frow;
      a_off[i][ks] = frag_off<KT>(r, ks, fhi);
    }
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int r = wn * WN + j * 32 + frow;
      b_off[j][ks] = BM * KT + frag_off<KT>(r, ks, fhi);
    }
  }
  // prologue: LOOK tiles in flight
#pragma unroll
  for (int s = 0; s < LOOK; ++s)
    if (kt_begin + s < kt_end) issue_tile(kt_begin + s, smem + s * TILE);
  DT(1);

  auto body = [&](auto CURc, int kt) {
    constexpr int CUR = decltype(CURc)::value;
    constexpr int NXT = (CUR + LOOK) % NSTAGE;
    // this wave's pieces of tile kt have landed once at most the pieces of the newer tiles in flight (LOOK-1 of them, fewer
    // at the end of the K range) are outstanding: a counted wait, the loads of the deeper stages keep flying
    auto wait_tiles = [&](auto Tc) {          // at most T newer K-tiles of this wave's pieces outstanding
      constexpr int T = decltype(Tc)::value;
      if (!RAGGED_B || nbw == NB) wait_vmcnt<T * (NA + NB)>();
      else if (nbw == NB - 1) wait_vmcnt<T * (NA + (NB > 1 ? NB - 1 : 0))>();
      else if (nbw == NB - 2) wait_vmcnt<T * (NA + (NB > 2 ? NB - 2 : 0))>();
      else wait_vmcnt<T * NA>();
    };
    if (LOOK >= 3 && kt + 2 < kt_end) wait_tiles(std::integral_constant<int, 2>{});
    else if (LOOK >= 2 && kt + 1 < kt_end) wait_tiles(std::integral_constant<int, 1>{});
    else wait_vmcnt<0>();
    loop_barrier();                                    // ... everyone's have; and everyone finished reading slot NXT
#ifdef DMA_TRACE
    if (kt - kt_begin < 8) DT(2 + (kt - kt_begin));
#endif
    const bf16_t* st = smem + CUR * TILE;
    bf16x8 af[2][FM], bfr[2][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i) af[0][i] = *(const bf16x8*)(st + a_off[i][0]);
#pragma unroll
    for (int j = 0; j < FN; ++j) bfr[0][j] = *(const bf16x8*)(st + b_off[j][0]);
    if (kt + LOOK < kt_end) issue_tile(kt + LOOK, smem + NXT * TILE);   // after the first fragment reads are in flight
#pragma unroll
    for (int ks = 0; ks < KT / 16; ++ks) {
      const int c = ks & 1, n = c ^ 1;
      if (ks + 1 < KT / 16) {
#pragma unroll
        for (int i = 0; i < FM; ++i) af[n][i] = *(const bf16x8*)(st + a_off[i][ks + 1]);
#pragma unroll
        for (int j = 0; j < FN; ++j) bfr[n][j] = *(const bf16x8*)(st + b_off[j][ks + 1]);
      }
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[c][i], bfr[c][j], acc[i][j], 0, 0, 0);
    }
  };
  {
    int kt = kt_begin;
    for (; kt + NSTAGE <= kt_end; kt += NSTAGE) {
      body(std::integral_constant<int, 0>{}, kt);
      body(std::integral_constant<int, 1>{}, kt + 1);
      if (NSTAGE >= 3) body(std::integral_constant<int, 2 % NSTAGE>{}, kt + 2);
      if (NSTAGE >= 4) body(std::integral_constant<int, 3 % NSTAGE>{}, kt + 3);
    }
    if (kt < kt_end) { body(std::integral_constant<int, 0>{}, kt); ++kt; }
    if (kt < kt_end) { body(std::integral_constant<int, 1>{}, kt); ++kt; }
    if (NSTAGE >= 4 && kt < kt_end) { body(std::integral_constant<int, 2 % NSTAGE>{}, kt); ++kt; }
  }
  DT(10);
  __syncthreads();   // all fragment reads done before the epilogue reuses the LDS
  DT(11);
#ifdef DMA_TRACE
  write_tile<WM, WN, FM, FN, GENERAL, EPI>(p, acc, wave_stage<WM, WN>(smem, wave), lane, m0 + wm * WM, n0 + wn * WN, dt_on ? g_dma_trace + dt_wg * 16 : nullptr);
#else
  if constexpr (NW * WM * (WN + 8) > NSTAGE * TILE || WM >= 128) {
    // tall wave tiles (the 4-wave 256-row variants): two row halves, so that the staging fits the operand buffers and the
    // (fully unrolled) epilogue stays at the size of the other kernels'
    static_assert(FM % 2 == 0 && NW * (WM / 2) * (WN + 8) <= NSTAGE * TILE, "epilogue staging must fit");
    write_tile<WM / 2, WN, FM / 2, FN, GENERAL, EPI>(p, *(f32x16(*)[FM / 2][FN])(acc + 0), wave_stage<WM / 2, WN>(smem, wave), lane, m0 + wm * WM, n0 + wn * WN);
    __syncthreads();
    write_tile<WM / 2, WN, FM / 2, FN, GENERAL, EPI>(p, *(f32x16(*)[FM / 2][FN])(acc + FM / 2), wave_stage<WM / 2, WN>(smem, wave), lane, m0 + wm * WM + WM / 2, n0 + wn * WN);
  } else {
    write_tile<WM, WN, FM, FN, GENERAL, EPI>(p, acc, wave_stage<WM, WN>(smem, wave), lane, m0 + wm * WM, n0 + wn * WN);
  }
  // tail rows: only in the 128 x 160 instantiations (and the ping-pong kernels), which have the registers for its 16 loads in flight — inlined
  // into the 64 / 128 / 256 x 128 tiles it cost them an occupancy step (92 -> 162 VGPRs on the 128 x 128 tile); the planner knows (plan_gemm_tail)
  if constexpr (MODE == 0 && BN == 160) {
    static_assert(NSTAGE * TILE * 2 >= NW * 16 * 64 * 4, "tail reduction must fit the operand buffers");
    if (p.tail_rows) gemm_tail<NW, GENERAL>(p, (float*)smem, wave, lane);      // (its first barrier orders it behind the staging reads above)
  }
#endif
  DT(12);
