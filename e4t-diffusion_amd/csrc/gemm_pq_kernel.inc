// Body of gemm_pq_kernel / gemm_pq_geglu_kernel (gemm.hip), included once into each (see gemm_dma_kernel.inc): the including kernel binds MODE, BN,
// GENERAL, EPI; `p` is its GemmArgs.
  constexpr int BM = 256, HK = 32;
  constexpr int WR = BN == 320 ? 4 : 2, WC = 8 / WR;
  constexpr int WM = BM / WR, WN = BN / WC;                  // 128 x 64 | 64 x 160
  constexpr int FM = WM / 32, FN = WN / 32;                  // 4 x 2 | 2 x 5
  constexpr int QA = BM * HK, QB = BN * HK;                  // elements per A / B quarter
  constexpr int HALF = QA + QB, BUF = 2 * HALF;              // [A | B] of one k half; one buffer = lo half + hi half
  constexpr int NBP = BN / 16;                               // B pieces per quarter: 16 | 20
  constexpr int NBJ = (NBP + 7) / 8;                         // per wave: 2 | 3 (the last one only in waves < NBP - 8 * (NBJ - 1))
  constexpr int NBLAST = NBP - 8 * (NBJ - 1);                // waves that carry NBJ pieces: 8 | 4
  constexpr int ESTG = 8 * 32 * (WN + 8);                    // epilogue staging: 8 waves x 32 rows
  static_assert(BN == 256 || BN == 320, "tile width");
  static_assert(2 * BUF * 2 <= 160 * 1024 && ESTG <= 2 * BUF, "LDS budget");
  __shared__ __attribute__((aligned(16))) bf16_t smem[2 * BUF];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wave >> 2;
  const int wr = wave / WC, wc = wave % WC;
  int tile_x, tile_y;
  xcd_tile(tile_x, tile_y, p.group_m);
  int m0 = tile_y * BM;
  const int n0 = tile_x * BN;
  const int mrows = p.M - m0;                       // valid (logical) rows of this tile
  if (p.panel_rows) m0 = (m0 / p.panel_rows) * p.panel_stride + p.panel_off + m0 % p.panel_rows;      // physical first row (panel_rows % 256 == 0)

  const int nkt = p.K / BK;
  const int bz = blockIdx.z / p.splitk, sz = blockIdx.z - bz * p.splitk;      // not batch_entry(): above the parent's time with it, profiles/gemm_addressing_ab.txt
  p.A += bz * p.strideA;
  if (p.A2) p.A2 += bz * p.strideA;
  p.B += bz * p.strideB;
  if (p.bias) p.bias += bz * p.strideBias;
  if (!p.reduce_batch) {
    if (p.flags & E4T_OUT_F32) p.C = (float*)p.C + bz * p.strideC;
    else p.C = (bf16_t*)p.C + bz * p.strideC;
  }
  const int kt_begin = sz * p.ktiles_per_split;
  int kt_end = kt_begin + p.ktiles_per_split;
  if (kt_end > nkt) kt_end = nkt;

  const bool cm = MODE != 0 && p.chan_major;          // channel-chunk-major K order (gemm_common.h, cm_step)
  const __amdgpu_buffer_rsrc_t rs_a = cm ? cm_rsrc(p) : __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, (int)p.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_a2 = __builtin_amdgcn_make_buffer_rsrc((void*)(p.A2 ? p.A2 : p.A), 0, (int)(p.A2 ? p.a2_bytes : p.a_bytes), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc((void*)p.B, 0, (int)p.b_bytes, 0x00020000);
  // DMA: one wave-instruction = 16 rows x 64 B; wave w feeds A rows 32w + 16j + (lane >> 2), j = 0, 1, and B pieces w + 8j
  const int drow = lane >> 2, dslot = lane & 3;
  long long a_base[2];
  int a_oy[2], a_ox[2], a_kc[2];
  bool a_ok[2];
  unsigned b_vo[NBJ];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int r = wave * 32 + j * 16 + drow;
    a_kc[j] = (dslot ^ ((r >> 2) & 3)) * 8;      // written out: profiles/gemm_addressing_isa.txt
    const int gr = m0 + r;
    a_ok[j] = r < mrows;
    if (MODE == 0) {
      a_base[j] = (long long)gr; a_oy[j] = a_ox[j] = 0;
    } else {
      out_pixel(p, gr, a_base[j], a_oy[j], a_ox[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < NBJ; ++j) {
    const int r = (wave + 8 * j) * 16 + drow;
    const int kc = (dslot ^ ((r >> 2) & 3)) * 8;
    const int gn = EPI == EPI_GEGLU ? geglu_col<WN>(n0, r, p.N) : n0 + r;
    b_vo[j] = (r < BN && gn < p.N) ? (unsigned)(((size_t)gn * p.ldb + kc) * 2) : OOB;
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
  int a_so = 0, b_so = 0;
  bool a_second = false;
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
  // the A and B streams are each issued in increasing k: lo(t), hi(t), lo(t+1), ...
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
    for (int j = 0; j < NBJ; ++j)
      if (j < NBJ - 1 || wave < NBLAST) buf_dma16(rs_b, b_vo[j], b_so, dst + ((wave + 8 * j) * 16) * HK);
    if (cm && hi) wb.next(BK);
  };
  // at most the 3 newest quarters of this wave outstanding: 2 A + 1 B after an even phase, 1 A + 2 B after an odd one
  constexpr int NBW_HI = NBJ, NBW_LO = NBJ - 1;
  auto wait3 = [&](auto ODDc) {
    constexpr bool ODD = decltype(ODDc)::value;
    if (NBLAST == 8 || wave < NBLAST) wait_vmcnt<(ODD ? 2 + 2 * NBW_HI : 4 + NBW_HI)>();
    else wait_vmcnt<(ODD ? 2 + 2 * NBW_LO : 4 + NBW_LO)>();
  };

  f32x16 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int frow = lane & 31, fhi = lane >> 5;
  int a_off[FM][2], b_off[FN][2];     // fragment offsets inside a quarter (elements), [block][k step of the half]
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int r = wr * WM + i * 32 + frow;
      a_off[i][ks] = r * HK + (((ks * 2 + fhi) ^ ((r >> 2) & 3)) * 8);
    }
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int r = wc * WN + j * 32 + frow;
      b_off[j][ks] = QA + r * HK + (((ks * 2 + fhi) ^ ((r >> 2) & 3)) * 8);
    }
  }
  // buffer b = smem + b * BUF: [lo: A | B][hi: A | B].  Prologue: lo(t0), hi(t0), B-lo(t0+1), A-lo(t0+1) — the stream position the
  // first phase expects (its own issue is A-lo(t+2)... of the NEXT tile: see the phase schedule).
  issue_b(kt_begin, false, smem + QA);
  issue_a(kt_begin, false, smem);
  issue_b(kt_begin, true, smem + HALF + QA);
  issue_a(kt_begin, true, smem + HALF);
  if (kt_begin + 1 < kt_end) {
    issue_b(kt_begin + 1, false, smem + BUF + QA);
    issue_a(kt_begin + 1, false, smem + BUF);
  }
  wait_vmcnt<0>();                 // (one-off: the first K-tile and the next one's lo half)
  __builtin_amdgcn_s_barrier();

  auto phase = [&](auto Bc, auto Pc, int kt) {
    constexpr int b = decltype(Bc)::value, ph = decltype(Pc)::value;
    constexpr int kh = ph >> 1, ks = ph & 1;
    bf16_t* const buf = smem + b * BUF;
    bf16_t* const other = smem + (b ^ 1) * BUF;
    const bf16_t* const q = buf + kh * HALF;
    bf16x8 af[FM], bfr[FN];
    // ---- L segment ----
#pragma unroll
    for (int i = 0; i < FM; ++i) af[i] = *(const bf16x8*)(q + a_off[i][ks]);
#pragma unroll
    for (int j = 0; j < FN; ++j) bfr[j] = *(const bf16x8*)(q + b_off[j][ks]);
    bool staged;
    if (ph == 0)      { staged = kt + 1 < kt_end && kt > kt_begin; if (staged) issue_a(kt + 1, false, other); }       // A-lo(t+1) (the prologue issued the first one)
    else if (ph == 1) { staged = kt + 1 < kt_end; if (staged) issue_b(kt + 1, true, other + HALF + QA); }              // B-hi(t+1)
    else if (ph == 2) { staged = kt + 1 < kt_end; if (staged) issue_a(kt + 1, true, other + HALF); }                   // A-hi(t+1)
    else              { staged = kt + 2 < kt_end; if (staged) issue_b(kt + 2, false, buf + QA); }                      // B-lo(t+2)
    if (staged) wait3(std::integral_constant<bool, (ph & 1) != 0>{}); else wait_vmcnt<0>();
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    // ---- M segment ----
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };
  using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>;

  if (grp == 1) __builtin_amdgcn_s_barrier();        // group 1 runs one barrier interval behind group 0
  {
    int kt = kt_begin;
    for (; kt + 2 <= kt_end; kt += 2) {
      phase(I0{}, I0{}, kt); phase(I0{}, I1{}, kt); phase(I0{}, I2{}, kt); phase(I0{}, I3{}, kt);
      phase(I1{}, I0{}, kt + 1); phase(I1{}, I1{}, kt + 1); phase(I1{}, I2{}, kt + 1); phase(I1{}, I3{}, kt + 1);
    }
    if (kt < kt_end) { phase(I0{}, I0{}, kt); phase(I0{}, I1{}, kt); phase(I0{}, I2{}, kt); phase(I0{}, I3{}, kt); }
  }
  if (grp == 0) __builtin_amdgcn_s_barrier();
  __syncthreads();   // every fragment read and every DMA is done before the epilogue reuses the LDS
  if (p.panel_rows) p.M = m0 + min(mrows, BM);      // the epilogue bounds PHYSICAL rows (never with split-K: p.M is the slab stride there)
  // 32-row slices of the wave tile: the staging of 8 waves x 32 x (WN + 8) fits the operand buffers, the unrolled epilogue stays small
  // (compile-time row index: a runtime-indexed accumulator array is placed in scratch memory — 704 bytes per lane written and read back
  // through HBM cost ~55 us per tile in the first version of this kernel)
  auto slice = [&](auto Ic) {
    constexpr int i = decltype(Ic)::value;
    write_tile<32, WN, 1, FN, GENERAL, EPI>(p, *(f32x16(*)[1][FN])(&acc[i][0]), wave_stage<32, WN>(smem, wave), lane, m0 + wr * WM + i * 32, n0 + wc * WN);
  };
  slice(I0{});
  __syncthreads();
  slice(I1{});
  if constexpr (FM == 4) {
    __syncthreads();
    slice(I2{});
    __syncthreads();
    slice(I3{});
  }
  if constexpr (MODE == 0) {
    if (p.tail_rows) gemm_tail<8, GENERAL>(p, (float*)smem, wave, lane);
  }
